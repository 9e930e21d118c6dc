"""The wave kernel keeps the primal residual of its interior-point phase as kappa * r_p0: r_p0 is written to LDS once, at the start of
the phase and again at a continuation after a failed refinement, and only the wave-uniform kappa moves (kappa <- (1 - alpha) kappa).
That is a change of representation: statuses, minimisers and iteration counts are those of the oracle and of the committed goldens.
The paths on which kappa is (re)set, one test each: the cold start (bench shape, all fixture states and the two edge cases), the
continuation (the degenerate N = 20 instances on the device; the one fixture state that takes it, on the host execution model), a
shape without a factored block (its totals take wave_sum2, and G'(d.r_p0) meets kappa straight from the MFMA pass), and the cold start
that follows a rejected warm start inside the closed loops."""
import os
import sys

import numpy as np
import pytest

import common
from LinearMPCOverNetworks import montecarlo
from oracle.oracle import Oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "wavesim"))

ATOL_U = 1e-8          # tests/test_hip_parity.py
S = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
# The one fixture state whose interior-point phase is entered a second time (refinement not certified -> continuation with r_p formed
# anew and kappa = 1): found with a host build of the kernel source that counts the entries (-DTMPC_ITERS_TOTAL) over all 600 states.
CONTINUATION_STATE = 587


@pytest.mark.gpu
def test_bench_shape_fixture_and_edge_cases(hip_lib, oracle_lib):
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True)
    assert hip_lib.kernel_name(mpc._handle) == "tmpc::solve_kernel<11,1,0,5,4,0,8>"
    gold = np.load(os.path.join(common.GOLDEN, "cartpole_N10_oracle.npz"))
    X = np.r_[S[:, :4], [[0.0, 0.0, 0.2, 0.0], [0.5, 0.0, 0.0, 0.0]]]      # + infeasible, + unconstrained
    R = np.r_[S[:, 4:], [[0.5, 0, 0, 0.0], [0.5, 0, 0, 0.0]]]
    ref = Oracle(mpc._problem_dict()).solve(X, R)
    assert list(ref["status"][-2:]) == [2, 0] and np.all(ref["status"][:600] == 0)
    out = mpc._solve(X, R)
    assert np.array_equal(out["status"], ref["status"])
    ok = ref["status"] == 0
    err, err_gold = np.max(np.abs(out["u_nom"][ok] - ref["u_nom"][ok])), np.max(np.abs(out["u_nom"][:600] - gold["u_nom"]))
    print(f"bench shape: max |u_nom - oracle| {err:.2e}, max |u_nom - golden| {err_gold:.2e}, mean iterations {out['iters'][:600].mean():.3f} "
          f"(oracle {ref['iters'][:600].mean():.3f})")
    assert err <= ATOL_U and err_gold <= ATOL_U
    assert np.all(np.isnan(out["u_nom"][600])) and out["iters"][601] == 0
    assert abs(out["iters"][:600].mean() - ref["iters"][:600].mean()) < 2.0 and out["iters"].max() < 40
    again = mpc._solve(X, R)
    for k in ("u_nom", "x_nom0", "xu_ss", "x_nom", "status", "iters"):
        assert np.array_equal(out[k], again[k], equal_nan=True), k


@pytest.mark.gpu
def test_continuation_resets_the_scale_on_the_hard_N20_states(hip_lib, oracle_lib):
    """tests/golden/cartpole_N20_extended_hard_states.npy: solves that go through failed refinements and continuations.  With the arrival
    flag of the file (what tests/test_full_size.py asks of them): all certified, u*_0 within 1e-8 of the oracle.  With the other problem of
    the controller: the oracle's verdicts, and its u*_0 where it has one."""
    D = np.load(os.path.join(common.GOLDEN, "cartpole_N20_extended_hard_states.npy"))
    X, R, G = np.ascontiguousarray(D[:, :4]), np.ascontiguousarray(D[:, 4:8]), D[:, 8].astype(np.uint8)
    mpc, _ = common.make_mpc("cartpole", 20, True, extended=True, create=True)
    orc = Oracle(mpc._problem_dict())
    for gam, own in ((G, True), ((1 - G).astype(np.uint8), False)):
        out = mpc._solve(X, R, gam, want_traj=False)
        ref = orc.solve(X, R, gam)
        assert np.array_equal(out["status"], ref["status"]), (own, out["status"], ref["status"])
        if own:
            assert np.all(out["status"] == 0), out["status"]
        ok = ref["status"] == 0
        assert np.all(np.isnan(out["u_nom"][ref["status"] == 2]))
        if ok.any():
            err = np.max(np.abs(out["u_nom"][ok, 0] - ref["u_nom"][ok, 0]))
            print(f"hard N = 20 states, {'own' if own else 'other'} problem: {ok.sum()} optimal, max |u*_0 - oracle| {err:.2e}")
            assert err <= ATOL_U


def test_continuation_state_of_the_fixture_on_the_host_model(oracle_lib):
    """CPU: the kernel's source on the host execution model (tests/wavesim).  State CONTINUATION_STATE of the N = 10 fixture is the
    only one of the 600 whose first hand-over is not certified; it must come back solved.  The bench shape parks the iterate of the
    hand-over in LDS (WaveLds::PARK_LDS: 884 idle words against the 642 it needs), so the host model, which has no save slot in HBM,
    CONTINUES the interior-point phase from that iterate -- r_p formed anew, kappa = 1 -- instead of running it again from its start.
    (The binary reports no count of the entries: that this state takes the path is known from the counting build named above, and
    would have to be found again if the fixture or the hand-over tolerance moved.)  A host build that fails is a failure of this test:
    the source it compiles is the kernel's."""
    import run_case
    binary = run_case.build_all()["wavesim"]
    mpc, _ = common.make_mpc("cartpole", 10, True, create=False)
    d = mpc._problem_dict()
    ii = [CONTINUATION_STATE]
    o = run_case.run(binary, d, S[ii, :4], S[ii, 4:])
    ref = Oracle(d).solve(S[ii, :4], S[ii, 4:])
    assert o["status"][0] == 0 == ref["status"][0]
    assert np.max(np.abs(o["u_nom"] - ref["u_nom"])) <= ATOL_U


@pytest.mark.gpu
def test_dense_single_shape_without_a_factored_block(hip_lib, oracle_lib):
    """Double integrator, N = 5, free x_0: the instances of tests/test_wavesim.py's edge-case test (feasible, trivially optimal, infeasible)."""
    mpc, _ = common.make_mpc("double_integrator", 5, False, create=True)
    assert hip_lib.kernel_name(mpc._handle) == "tmpc::solve_kernel<8,0,2,0,0,0,8>"
    rng = np.random.default_rng(4)
    X = np.r_[rng.uniform(-1, 1, (20, 2)) * [7.5, 0.9], [[0.0, 0.0]], [[30.0, 0.0]], [[-3.1437307257161446, 0.5378281719126672]]]
    R = np.c_[np.r_[rng.uniform(-9, 9, 20), 0.0, 0.0, 4.697848229977945], np.zeros(len(X))]
    ref = Oracle(mpc._problem_dict()).solve(X, R)
    assert 0 in ref["status"] and 2 in ref["status"] and ref["iters"][20] == 0
    out = mpc._solve(X, R)
    assert np.array_equal(out["status"], ref["status"]), (out["status"], ref["status"])
    ok = ref["status"] == 0
    assert np.max(np.abs(out["u_nom"][ok] - ref["u_nom"][ok])) <= ATOL_U
    assert np.all(np.isnan(out["u_nom"][~ok])) and np.all(np.isnan(out["xu_ss"][~ok])) and out["iters"][20] == 0


@pytest.mark.gpu
def test_cold_start_after_a_rejected_warm_start_in_the_closed_loops(hip_lib):
    """64 trajectories x 12 steps at p_loss 0.3, warm-started.  The reference steps at t = 6: the working set of t = 5 is rejected there and
    the cold start follows in the same solve.  One fused launch equals the launch pair per step bit for bit, and the step costs
    interior-point iterations that the same loop with a constant reference does not spend."""
    nb, T = 64, 12
    mpc, w = common.make_mpc("cartpole", 10, True, create=True)
    p_loss = np.full(nb, 0.3)
    th, ga, dist = montecarlo.draw_realisations(nb, T, w["w_bound"], seed=17)
    ref = np.where(np.arange(T) < 6, 0.5, -0.3)
    off = mpc.run_closed_loop(p_loss, ref, th, ga, dist, warm_start=True, capture=5, fused="off")
    on = mpc.run_closed_loop(p_loss, ref, th, ga, dist, warm_start=True, capture=5, fused="on")
    assert on["fused"] and not off["fused"]
    for k in ("err2", "tube_violations", "not_optimal", "x_final", "consistent", "iters_sum", "x_traj", "x_nom_traj", "u_traj"):
        assert np.array_equal(np.asarray(on[k]), np.asarray(off[k]), equal_nan=True), k
    assert np.all(on["not_optimal"] == 0) and np.all(on["tube_violations"] == 0)
    flat = mpc.run_closed_loop(p_loss, 0.5 * np.ones(T), th, ga, dist, warm_start=True, fused="on")
    print(f"warm closed loop: iterations per trajectory {on['iters_sum'].mean():.1f} with the reference step, {flat['iters_sum'].mean():.1f} without")
    assert on["iters_sum"].sum() > flat["iters_sum"].sum()
