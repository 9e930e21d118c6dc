"""The whole device loop -- solver and state machines -- with several inputs.  Every other closed-loop test runs the
cart-pole (nx = 4, nu = 1) or the double integrator (nx = 2, nu = 1), where row-major and column-major B, K, K_anc coincide
and the packet, capture and trace strides hide a swapped index; tests/test_device_glue_shapes.py judges the state machines
alone against a naive reference, here they run behind real solves:

* BASELINE config 5 (synthetic, nx = 12, nu = 4, N = 30) on the workgroup-per-QP kernel: tmpc_mc_run against
  montecarlo.run_remote_tube_mpc driven by the same handle's solves, with host draws and with the device generator
  (Philox blocks 2 and 3 of a step);
* a two-input model (nx = 3, nu = 2, N = 5) whose QPs take wave-per-QP shapes: the same comparison, closed_loop_kernel
  (fused) against the launch pair per step bit for bit, and closed_loop_step_kernel for the extended controller;
* a RegulatorMPC and a TubeRegulatorMPC with nx = 3, nu = 2, full Q and R and an input polytope that couples the inputs:
  tmpc_reg_run against regulator_problems.host_loop.

The bands are the project's for these comparisons (tests/test_closed_loop.py: test_device_resident_loop_equals_host_loop;
regulator_problems.compare_loops)."""
import numpy as np
import pytest

import common
import regulator_problems as rp
from LinearMPCOverNetworks import _native, montecarlo
from LinearMPCOverNetworks.polytope_lite import Polytope, as_polytope, box2poly
from LinearMPCOverNetworks.RegulatorMPC import RegulatorMPC
from LinearMPCOverNetworks.TubeRegulatorMPC import TubeRegulatorMPC
from LinearMPCOverNetworks.TubeTrackingMPC import ExtendedTubeTrackingMPC, TubeTrackingMPC

P_LOSS = np.tile([0.0, 0.3, 0.6, 0.9], 4)          # B = 16
NB, T = 16, 12
KEYS = ("err2", "tube_violations", "not_optimal", "x_final", "consistent", "iters_sum", "x_traj", "x_nom_traj", "u_traj")   # test_shape_parity.KEYS


def _host_loop(mpc, w, p_loss, ref, th, ga, dist, extended, capture, seen=None):
    obs = None if seen is None else (lambda t, st: seen.append(t - st["s"]))
    return montecarlo.run_remote_tube_mpc(mpc.determine_packets, w["A"], w["B"], mpc.get_steady_state_controller_gain(),
                                          mpc.get_ancillary_controller_gain(), mpc._N, mpc._Z, p_loss, ref, th, ga, dist,
                                          extended=extended, capture=capture, observer=obs)


def _compare(label, dev, host):
    """The bands of test_device_resident_loop_equals_host_loop, and the captured sample run to 1e-8."""
    fig = {k: float(np.max(np.abs(dev[k] - host[k]))) for k in ("x_final", "tracking_error", "x_traj", "x_nom_traj", "u_traj")}
    print(f"   {label}: max |device loop - host loop|: " + ", ".join(f"{k} {v:.1e}" for k, v in fig.items()))
    assert np.array_equal(dev["not_optimal"], host["not_optimal"]) and np.all(dev["not_optimal"] == 0)
    assert np.array_equal(dev["tube_violations"], host["tube_violations"]) and np.all(dev["tube_violations"] == 0)
    assert fig["x_final"] <= 1e-8 and fig["tracking_error"] <= 1e-10
    assert max(fig["x_traj"], fig["x_nom_traj"], fig["u_traj"]) <= 1e-8


def _device_vs_host(label, mpc, w, ref, extended, seed):
    """Host draws, then the device generator against the host loop fed with its twin's arrays; trajectory 7 (p = 0.9) captured."""
    th, ga, dist = montecarlo.draw_realisations(NB, T, w["w_bound"], seed=seed)
    seen = []
    host = _host_loop(mpc, w, P_LOSS, ref, th, ga, dist, extended, 7, seen)
    dev = mpc.run_closed_loop(P_LOSS, ref, th, ga, dist, extended=extended, capture=7)
    _compare(label + ", host draws", dev, host)
    assert np.array(seen).max() >= 1 and np.abs(host["u_traj"]).max() > 1e-3         # later columns of a packet reach the plant
    thp, gap, distp = montecarlo.draw_realisations_philox(NB, T, w["w_bound"], seed=seed, first=500)
    host = _host_loop(mpc, w, P_LOSS, ref, thp, gap, distp, extended, 7)
    dev = mpc.run_closed_loop(P_LOSS, ref, extended=extended, capture=7, device_rng=(seed, 500, w["w_bound"]))
    _compare(label + ", device generator", dev, host)
    # and, as tests/test_device_rng.py has it for the cart-pole: device draws = the twin's arrays handed in, bit for bit
    arrays = mpc.run_closed_loop(P_LOSS, ref, thp, gap, distp, extended=extended, capture=7)
    for k in ("err2", "tube_violations", "not_optimal", "x_final", "iters_sum", "x_traj", "x_nom_traj", "u_traj"):
        np.testing.assert_array_equal(dev[k], arrays[k], err_msg=k)


# ------------------------------------------------------------------------------------------------ config 5, block kernel
@pytest.mark.gpu
def test_config5_device_loop_equals_host_loop(hip_lib):
    mpc, w = common.make_mpc("synthetic", 30, True, create=True)
    try:
        assert (mpc._nx, mpc._nu) == (12, 4) and mpc.get_kernel_path() == "block"
        ref = np.where(np.arange(T) < T // 2, 1.0, -0.6)
        _device_vs_host("config 5 (nx 12, nu 4, N 30), block kernel", mpc, w, ref, False, seed=55)
    finally:
        mpc._close()


# ------------------------------------------------------------------------------------------------ two inputs, wave kernels
TWO_N = 5
# what the two-input problems reach (tmpc_kernel_name) and their condensed sizes (nv, rows), as tests/shape_cases.py records
# its cases: a drift of the sets or of the shape table shows here
TWO_KERNELS = {False: [("tmpc::solve_kernel<12,1,0,5,4,0,8>", (12, 182))],
               True: [("tmpc::solve_kernel<12,1,0,5,4,0,8>", (12, 182)), ("tmpc::solve_kernel<16,0,4,0,0,0,4>", (15, 141))]}
_TWO_SETS = {}


def two_input_model():
    """nx = 3, nu = 2: dense, non-symmetric A and B (every entry of B at its own place in either layout)."""
    A = np.array([[1.0, 0.5, 0.0], [0.0, 1.0, 0.3], [0.1, 0.0, 0.8]])
    B = np.array([[0.0, 0.1], [0.5, 0.0], [0.2, 1.0]])
    wb = 0.05 * np.ones(3)
    return dict(A=A, B=B, Q=np.eye(3), R=np.eye(2), X=box2poly([[-8.0, 8.0]] * 3), U=box2poly([[-1.0, 1.0]] * 2),
                W=box2poly(np.c_[-wb, wb]), w_bound=wb)


def two_input_mpc(extended, device):
    """The controller with its sets computed once (scipy back-end: tests/conftest.py) on a host-only handle."""
    w = two_input_model()
    if not _TWO_SETS:
        m = ExtendedTubeTrackingMPC(w["A"], w["B"], w["Q"], w["R"], TWO_N)
        m.set_input_constraints(w["U"])
        m.set_state_constraints(w["X"])
        m.set_device(-1)
        m.setup_optimization(w["W"], fixed_initial_state=True, rpi_method=1)
        _TWO_SETS.update(m.export_sets())
        m._close()
    sets = dict(_TWO_SETS)
    if not extended:
        sets.pop("ZmW_A"), sets.pop("ZmW_b"), sets.pop("XfP_A"), sets.pop("XfP_b")
    mpc = (ExtendedTubeTrackingMPC if extended else TubeTrackingMPC)(w["A"], w["B"], w["Q"], w["R"], TWO_N)
    mpc.set_input_constraints(w["U"])
    mpc.set_state_constraints(w["X"])
    mpc.set_device(device)
    mpc.setup_from_sets(sets, fixed_initial_state=True, create=True)
    return mpc, w


@pytest.mark.parametrize("extended", [False, True])
def test_two_input_problems_take_wave_shapes(hip_lib, extended):
    mpc, _ = two_input_mpc(extended, device=-1)
    try:
        got = [(_native.kernel_name(mpc._handle, v), _native.get_dims(mpc._handle, v)[:2]) for v in range(1 + extended)]
        assert got == TWO_KERNELS[extended], got
    finally:
        mpc._close()


TWO_REF = np.where(np.arange(T) < T // 2, 2.0, -1.2)


@pytest.mark.gpu
@pytest.mark.parametrize("extended", [False, True])
def test_two_input_device_loop_equals_host_loop(hip_lib, extended):
    mpc, w = two_input_mpc(extended, device=0)
    try:
        assert [_native.kernel_name(mpc._handle, v) for v in range(1 + extended)] == [k for k, _ in TWO_KERNELS[extended]]
        _device_vs_host(f"two inputs (nx 3, nu 2, N {TWO_N}), wave kernels, extended = {extended}", mpc, w, TWO_REF, extended, seed=32)
    finally:
        mpc._close()


@pytest.mark.gpu
@pytest.mark.parametrize("extended,warm", [(False, False), (False, True), (True, False), (True, True)])
def test_two_input_fused_loops_equal_the_launch_pair_per_step(hip_lib, extended, warm):
    """closed_loop_kernel<shape> (one launch for the whole loop) and, for the extended controller, closed_loop_step_kernel<shape> of
    both problems against a solve launch + state-machine launch per step: bit for bit, as test_shape_parity.py::test_closed_loop_twins
    has it for one input."""
    mpc, w = two_input_mpc(extended, device=0)
    try:
        nb, steps = 40, 16
        p_loss = np.tile(np.arange(10) / 10.0, nb // 10)
        th, ga, dist = montecarlo.draw_realisations(nb, steps, w["w_bound"], seed=46)
        ref = np.where(np.arange(steps) < steps // 2, 2.0, -1.2)
        kw = dict(extended=extended, warm_start=warm, capture=3)
        off = mpc.run_closed_loop(p_loss, ref, th, ga, dist, fused="off", **kw)
        on = mpc.run_closed_loop(p_loss, ref, th, ga, dist, fused="on", **kw)
        assert off["loop_mode"] == 0 and on["loop_mode"] == (2 if extended else 1)
        for k in KEYS:
            assert np.array_equal(np.asarray(on[k]), np.asarray(off[k]), equal_nan=True), k
        assert on["iters_mean"] > 0.5 and np.all(on["not_optimal"] == 0) and np.abs(on["u_traj"]).max() > 1e-3
    finally:
        mpc._close()


# ------------------------------------------------------------------------------------------------ regulators, nx = 3, nu = 2
def _regulator(tube, device=0):
    w = two_input_model()
    Q = np.array([[2.0, 0.3, -0.2], [0.3, 1.0, 0.4], [-0.2, 0.4, 1.5]])
    R = np.array([[0.5, 0.2], [0.2, 0.8]])
    assert np.all(np.linalg.eigvalsh(Q) > 0) and np.all(np.linalg.eigvalsh(R) > 0)
    # |u_i| <= 1 and two rows that couple the inputs
    U = Polytope(np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0], [1.0, 1.0], [-1.0, 0.5]]), np.array([1.0, 1.0, 1.0, 1.0, 1.5, 1.2]))
    m = (TubeRegulatorMPC if tube else RegulatorMPC)(w["A"], w["B"], Q, R, 6)
    m.set_input_constraints(U)
    m.set_state_constraints(box2poly([[-4.0, 4.0]] * 3))
    m.set_device(device)
    if tube:
        # setup_optimization(W) step by step, with the Darup-Teichrib RPI set (105 rows, under a second; the default
        # construction gives 1155 rows after half a minute of LPs)
        m._W = as_polytope(w["W"])
        m.determine_mRPI(m._W, rpi_method=1)
        m.tighten_constraints()
        m.determine_Xf(verbose=False)
        m.generate_optimization_problem()
    else:
        m.generate_optimization_problem()
    return m, w


@pytest.mark.gpu
@pytest.mark.parametrize("tube", [False, True])
def test_two_input_regulator_device_loop_equals_host_loop(hip_lib, tube):
    m, w = _regulator(tube)
    try:
        nb, steps = 64, 15
        rng = np.random.default_rng(9)
        x0 = rng.uniform(-1.0, 1.0, (nb, 3)) * [4.6, 3.0, 3.0]           # some start outside X: they fail at step 0
        x0[0] = [1.0, -0.5, 0.8]                                         # the captured trajectory (host_loop records trajectory 0)
        dist = rng.uniform(-1.0, 1.0, (nb, steps, 3)) * w["w_bound"]
        sets = {"X": m._X, "U": m._U, "Z": m._Z} if tube else {"X": m._X, "U": m._U}
        K = m.get_controller_gain() if tube else None
        dev = m.run_closed_loop(x0, steps, w=dist, capture=0)
        host = rp.host_loop(m, x0, dist, sets, K)
        n_fail = int(np.sum(host["fail_step"] >= 0))
        print(f"   regulator nx 3, nu 2, tube = {tube}: {n_fail} of {nb} trajectories fail, "
              f"max |x_final(device) - x_final(host)| {float(np.max(np.abs(dev['x_final'] - host['x_final']))):.1e}, "
              f"max rel. cost difference {float(np.max(np.abs(dev['cost'] - host['cost']) / (1 + np.abs(host['cost'])))):.1e}")
        assert 0 < n_fail < nb
        assert np.abs(host["u_traj"][np.isfinite(host["u_traj"])]).max() > 1e-3 and host["cost"].max() > 1.0
        rp.compare_loops(dev, host)
        # check sets small enough that the counters count (inside U and X they stay at zero whatever the row layout)
        tight = dict(sets, U=Polytope(m._U.A, 0.2 * m._U.b), X=box2poly([[-0.5, 0.5]] * 3))
        host = rp.host_loop(m, x0, dist, tight, K)
        assert host["u_viol"].max() >= 2 and host["x_viol"].max() >= 2 and (host["u_viol"] == 0).any()
        rp.compare_loops(m.run_closed_loop(x0, steps, w=dist, check_sets=tight, capture=0), host)
        # the device generator against the same loop fed with its host twin's disturbances
        _, _, wp = montecarlo.draw_realisations_philox(nb, steps, w["w_bound"], seed=77, first=1000)
        dev = m.run_closed_loop(x0, steps, seed=77, first_trajectory=1000, w_bound=w["w_bound"], capture=0)
        rp.compare_loops(dev, rp.host_loop(m, x0, wp, sets, K))
    finally:
        m._close()


@pytest.mark.gpu
def test_wide_regulator_device_generator_equals_host_twin(hip_lib):
    """nx = 12, nu = 4 (the model of config 5, N = 5): reg_step_kernel draws w_2 .. w_11 from Philox blocks 1, 2 and 3 of the step;
    the loop fed by the device generator against the host loop fed with draw_realisations_philox."""
    w = common.workload("synthetic")
    m = RegulatorMPC(w["A"], w["B"], w["Q"], w["R"], 5)
    m.set_input_constraints(w["U"])
    m.set_state_constraints(w["X"])
    m.generate_optimization_problem()
    try:
        nb, steps = 32, 10
        x0 = np.random.default_rng(12).uniform(-2.0, 2.0, (nb, 12))
        x0[-4:, 0] = 12.0                                             # outside X: these fail at step 0
        wb = 0.01 * (1.0 + np.arange(12))
        dev = m.run_closed_loop(x0, steps, seed=78, first_trajectory=40, w_bound=wb, capture=0)
        _, _, wp = montecarlo.draw_realisations_philox(nb, steps, wb, seed=78, first=40)
        host = rp.host_loop(m, x0, wp, {"X": m._X, "U": m._U}, None)
        n_fail = int(np.sum(host["fail_step"] >= 0))
        print(f"   regulator nx 12, nu 4: {n_fail} of {nb} trajectories fail, "
              f"max |x_final(device) - x_final(host)| {float(np.max(np.abs(dev['x_final'] - host['x_final']))):.1e}")
        assert 4 <= n_fail < nb and host["fail_step"][0] < 0
        rp.compare_loops(dev, host)
        # the disturbance matters at this band: without it the final states differ by far more than 1e-12
        assert np.max(np.abs(m.run_closed_loop(x0, steps)["x_final"] - dev["x_final"])) > 1e-3
    finally:
        m._close()
