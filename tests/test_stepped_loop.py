"""The stepped closed loop around a plant of the caller's (include/tmpc.h: tmpc_mc_open / tmpc_mc_step_device / tmpc_mc_step /
tmpc_mc_close; TubeTrackingMPC.open_closed_loop) on the device.  Bands: the project's own for the device loop against the host
loop (tests/test_closed_loop.py: integers equal, tracking_error to 1e-10, final states to 1e-8); where the same arithmetic runs
twice, bytes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import common
from LinearMPCOverNetworks import _native, montecarlo, workloads
from LinearMPCOverNetworks.polytope_lite import Polytope
from test_stepped_loop_api import E_INVALID, raw_open

pytestmark = pytest.mark.gpu

NB, T = 19, 40                                        # 19: no multiple of any waves-per-workgroup
P_LOSS = np.tile([0.0, 0.3, 0.9], 7)[:NB]
REF = np.where(np.arange(T) < T // 2, 0.5, -0.3)      # the reference steps on the way
SEED = 23
_MPC = {}


def _cartpole(extended):
    """The cart-pole controller at N = 10 (shapes (11,1,0,5,4,0) and, extended, (15,1,0,4,7,0)), one per module run."""
    if extended not in _MPC:
        _MPC[extended] = common.make_mpc("cartpole", 10, True, extended=extended, create=True)
    return _MPC[extended]


def _draws(w, nb=NB, nt=T, seed=SEED):
    return montecarlo.draw_realisations(nb, nt, w["w_bound"], seed=seed)


def _linear(w):
    A, B = np.asarray(w["A"], dtype=np.float64), np.asarray(w["B"], dtype=np.float64)
    return lambda x, u: x @ A.T + u @ B.T


def _session(mpc, plant, p_loss, ref, th, ga, dist, extended=False, x0=None, feed=None, **kw):
    """A session stepped through the host-pointer entry around plant(x, u) + dist[:, t].  feed = (c, x_traj): trajectory c gets
    x_traj[t] instead of its plant's state.  Returns the statistics, plus x_final, and every x_t / u_t as x_all / u_all (T, B, .)."""
    nb, nt = th.shape
    x = np.zeros((nb, mpc._nx)) if x0 is None else np.array(x0, dtype=np.float64)
    xs, us = [], []
    with mpc.open_closed_loop(p_loss, ref, th, ga, x0=x0, extended=extended, **kw) as s:
        for t in range(nt):
            if feed is not None:
                x[feed[0]] = feed[1][t]
            u = s.step(x)
            xs.append(x.copy())
            us.append(u.copy())
            x = plant(x, u) + dist[:, t]
    out = dict(s.stats)
    out.update(x_final=x, x_all=np.array(xs), u_all=np.array(us))
    return out


def _host_loop(mpc, w, p_loss, ref, th, ga, dist, extended, plant=None, **kw):
    return montecarlo.run_remote_tube_mpc(mpc.determine_packets, w["A"], w["B"], mpc.get_steady_state_controller_gain(),
                                          mpc.get_ancillary_controller_gain(), mpc._N, mpc._Z, p_loss, ref, th, ga, dist,
                                          extended=extended, plant=plant, **kw)


def _compare(label, dev, ref):
    fig = {k: float(np.max(np.abs(dev[k] - ref[k]))) for k in ("x_final", "tracking_error")}
    print(f"   {label}: max |session - reference loop|: " + ", ".join(f"{k} {v:.1e}" for k, v in fig.items()))
    assert np.array_equal(dev["not_optimal"], ref["not_optimal"])
    assert np.array_equal(dev["tube_violations"], ref["tube_violations"])
    assert fig["tracking_error"] <= 1e-10 and fig["x_final"] <= 1e-8, fig


# ------------------------------------------------------------------------------------------------ 1: the host loop, linear plant
@pytest.mark.parametrize("extended", [False, True])
def test_session_equals_the_host_loop(hip_lib, extended):
    mpc, w = _cartpole(extended)
    th, ga, dist = _draws(w)
    host = _host_loop(mpc, w, P_LOSS, REF, th, ga, dist, extended)
    dev = _session(mpc, _linear(w), P_LOSS, REF, th, ga, dist, extended)
    assert dev["steps"] == T and np.all(dev["not_optimal"] == 0) and np.all(dev["tube_violations"] == 0)
    assert np.all(dev["x_violations"] == 0) and np.all(dev["u_violations"] == 0)          # no check set given
    _compare(f"cart-pole N 10, extended = {extended}", dev, host)
    if not extended:
        assert dev["consistent_estimate_error"] < 1e-9


# ------------------------------------------------------------------------------------------------ 2: tmpc_mc_run, bit for bit
@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("fused", ["off", None])
def test_session_fed_a_recorded_trajectory_repeats_the_run(hip_lib, extended, fused):
    """Trajectory c of a tmpc_mc_run, recorded, is fed to trajectory c of a session step by step: the same inputs and statistics,
    byte for byte, whatever the other trajectories of the batch do and whichever launch form the run took."""
    mpc, w = _cartpole(extended)
    th, ga, dist = _draws(w)
    for c in (0, 7, 17):                              # loss rates 0, 0.3, 0.9
        run = mpc.run_closed_loop(P_LOSS, REF, th, ga, dist, extended=extended, capture=c, fused=fused)
        dev = _session(mpc, _linear(w), P_LOSS, REF, th, ga, dist, extended, feed=(c, run["x_traj"]))
        assert dev["u_all"][:, c].tobytes() == run["u_traj"].tobytes(), (c, np.max(np.abs(dev["u_all"][:, c] - run["u_traj"])))
        for k in ("err2", "tube_violations", "not_optimal", "iters_sum"):
            assert dev[k][c:c + 1].tobytes() == run[k][c:c + 1].tobytes(), (c, k, dev[k][c], run[k][c])


def test_warm_started_session_equals_the_cold_one(hip_lib):
    mpc, w = _cartpole(False)
    th, ga, dist = _draws(w)
    cold = _session(mpc, _linear(w), P_LOSS, REF, th, ga, dist)
    warm = _session(mpc, _linear(w), P_LOSS, REF, th, ga, dist, warm_start=True)
    assert np.all(cold["not_optimal"] == 0) and np.all(warm["not_optimal"] == 0)
    assert np.array_equal(cold["tube_violations"], warm["tube_violations"])
    np.testing.assert_allclose(warm["x_final"], cold["x_final"], atol=1e-8, rtol=0)               # tests/test_closed_loop.py:267-268
    np.testing.assert_allclose(warm["tracking_error"], cold["tracking_error"], atol=1e-10, rtol=0)
    print(f"   interior-point iterations of the session: cold {cold['iters_sum'].sum()}, warm {warm['iters_sum'].sum()}")
    assert warm["iters_sum"].sum() < cold["iters_sum"].sum()
    again = _session(mpc, _linear(w), P_LOSS, REF, th, ga, dist)                                   # the setting is per session
    assert np.array_equal(again["iters_sum"], cold["iters_sum"])


# ------------------------------------------------------------------------------------------------ 3: a nonlinear plant
def test_session_around_the_nonlinear_cartpole_equals_the_device_plant(hip_lib):
    mpc, w = _cartpole(False)
    nb, nt = 16, 50
    p_loss = np.tile([0.0, 0.3, 0.6, 0.9], 4)
    th, ga, dist = _draws(w, nb, nt, seed=31)
    dist = 0.0 * dist
    ref = 0.5 * np.ones(nt)
    dev_plant = mpc.run_closed_loop(p_loss, ref, th, ga, dist, plant="cartpole")
    ses = _session(mpc, lambda x, u: workloads.cartpole_step(x, u[:, 0]), p_loss, ref, th, ga, dist)
    _compare("nonlinear cart-pole, numpy RK4 outside against the device's RK4 inside", ses, dev_plant)
    lin = _session(mpc, _linear(w), p_loss, ref, th, ga, dist)
    assert np.max(np.abs(ses["x_final"] - lin["x_final"])) > 1e-6                                 # it really is another plant
    # the plant setting of the handle is neither used nor touched by a session
    again = mpc.run_closed_loop(p_loss, ref, th, ga, dist)
    np.testing.assert_allclose(again["x_final"], lin["x_final"], atol=1e-8, rtol=0)


# ------------------------------------------------------------------------------------------------ 4: device pointers, stream order
def test_device_pointer_steps_ordered_by_events_equal_synchronised_steps(hip_lib):
    """The plant as torch kernels on a stream of the caller's, no synchronisation inside the loop (an event each way per step),
    against the same loop with caller_stream = NULL and a device-wide / handle synchronisation around every step: bytes."""
    import torch
    mpc, w = _cartpole(True)
    h = mpc._handle
    th, ga, dist = _draws(w)
    dev = torch.device("cuda", 0)
    A = torch.as_tensor(np.asarray(w["A"], dtype=np.float64), device=dev)
    Bm = torch.as_tensor(np.asarray(w["B"], dtype=np.float64), device=dev)
    wd = torch.as_tensor(np.ascontiguousarray(dist.transpose(1, 0, 2)), device=dev)

    def loop(ordered):
        with torch.cuda.stream(torch.cuda.Stream(device=dev)):
            x = torch.zeros((NB, 4), dtype=torch.float64, device=dev)
            us = torch.zeros((T, NB, 1), dtype=torch.float64, device=dev)
            u_own = torch.zeros((NB, 1), dtype=torch.float64, device=dev)
            ses = mpc.open_closed_loop(P_LOSS, REF, th, ga, extended=True)
            for t in range(T):
                if ordered:
                    u = ses.step(x)
                else:
                    torch.cuda.synchronize()
                    _native.mc_step(h, ses._info, x.data_ptr(), u_own.data_ptr(), None)
                    _native.synchronize(h)
                    u = u_own
                us[t].copy_(u)
                x = (x @ A.T + u @ Bm.T + wd[t]).contiguous()
            torch.cuda.synchronize()
            stats = ses.close()
        return stats, us.cpu().numpy(), x.cpu().numpy()
    a_stats, a_u, a_x = loop(True)
    b_stats, b_u, b_x = loop(False)
    assert a_stats["steps"] == T and np.abs(a_u).max() > 1e-3
    assert a_u.tobytes() == b_u.tobytes() and a_x.tobytes() == b_x.tobytes()
    for k in ("err2", "tube_violations", "not_optimal", "iters_sum", "consistent"):
        assert a_stats[k].tobytes() == b_stats[k].tobytes(), k
    # and it is the loop of test 1
    host = _host_loop(mpc, w, P_LOSS, REF, th, ga, dist, True)
    a_stats["x_final"] = a_x
    _compare("torch plant on the caller's stream", a_stats, host)


def test_run_closed_loop_with_a_callable_plant(hip_lib):
    import torch
    mpc, w = _cartpole(False)
    th, ga, dist = _draws(w)
    A = torch.as_tensor(np.asarray(w["A"], dtype=np.float64), device="cuda")
    Bm = torch.as_tensor(np.asarray(w["B"], dtype=np.float64), device="cuda")
    out = mpc.run_closed_loop(P_LOSS, REF, th, ga, dist, plant=lambda x, u: x @ A.T + u @ Bm.T)      # on torch's default stream
    host = _host_loop(mpc, w, P_LOSS, REF, th, ga, dist, False)
    _compare("run_closed_loop(plant = callable)", out, host)


# ------------------------------------------------------------------------------------------------ 5: several inputs
@pytest.mark.parametrize("extended", [False, True])
def test_two_input_session_equals_the_host_loop(hip_lib, extended):
    from test_closed_loop_several_inputs import two_input_mpc
    mpc, w = two_input_mpc(extended, device=0)
    try:
        nb, nt = 9, 30
        p_loss = np.tile([0.0, 0.3, 0.9], 3)
        th, ga, dist = _draws(w, nb, nt, seed=32)
        ref = np.where(np.arange(nt) < nt // 2, 2.0, -1.2)
        host = _host_loop(mpc, w, p_loss, ref, th, ga, dist, extended)
        dev = _session(mpc, _linear(w), p_loss, ref, th, ga, dist, extended)
        assert np.all(dev["not_optimal"] == 0) and np.abs(dev["u_all"][:, :, 1]).max() > 1e-3     # the second input is in use
        _compare(f"two inputs (nx 3, nu 2, N 5), extended = {extended}", dev, host)
    finally:
        mpc._close()


# ------------------------------------------------------------------------------------------------ 6: the block kernel
def test_block_kernel_session_equals_the_host_loop(hip_lib):
    mpc, w = common.make_mpc("cartpole", 10, True, create=True)
    try:
        mpc.set_kernel_path("block")
        assert mpc.get_kernel_path() == "block"
        nb, nt = 5, 12
        p_loss = np.array([0.0, 0.3, 0.9, 0.3, 0.9])
        th, ga, dist = _draws(w, nb, nt, seed=6)
        ref = np.where(np.arange(nt) < nt // 2, 0.5, -0.3)
        host = _host_loop(mpc, w, p_loss, ref, th, ga, dist, False)
        dev = _session(mpc, _linear(w), p_loss, ref, th, ga, dist)
        assert np.all(dev["not_optimal"] == 0)
        _compare("block kernel", dev, host)
    finally:
        mpc._close()


# ------------------------------------------------------------------------------------------------ 7: R-MPC
def test_rmpc_session_stops_infeasible_trajectories_with_zero_input(hip_lib):
    """The scenario of tests/test_tracking_mpc.py::test_rmpc_closed_loop_device_equals_host (its first 64 trajectories)."""
    from test_tracking_mpc import _make
    mpc, w = _make(True)
    try:
        nb, nt = 64, 60
        rng = np.random.default_rng(11)
        x0 = (rng.uniform(-1, 1, (96, 2)) * [7.6, 0.6])[:nb]
        p_loss = np.tile([0.0, 0.3, 0.6, 0.9], nb // 4)
        th, ga, dist = montecarlo.draw_realisations(nb, nt, 3.0 * w["w_bound"], seed=5)
        ref = np.where(np.arange(nt) < 30, 6.0, -6.0)
        host = montecarlo.run_remote_tracking_mpc(mpc.determine_packets, w["A"], w["B"], mpc.get_steady_state_controller_gain(), 10,
                                                  p_loss, ref, th, ga, dist, x0=x0)
        dev = _session(mpc, _linear(w), p_loss, ref, th, ga, dist, x0=x0)
        dead = np.isnan(dev["tracking_error"])
        assert np.array_equal(dead, host["infeasible"]) and 0 < dead.sum() < nb
        assert np.array_equal(dev["not_optimal"], host["not_optimal"])
        live = ~dead
        np.testing.assert_allclose(dev["tracking_error"][live], host["tracking_error"][live], atol=1e-10, rtol=0)
        np.testing.assert_allclose(dev["x_final"][live], host["x_final"][live], atol=1e-8, rtol=0)
        # a stopped trajectory: its plant state of the host loop freezes at the failing step -- and from that step on u_t = 0
        for b in np.flatnonzero(dead):
            zero = np.all(dev["u_all"][:, b] == 0.0, axis=1)
            assert zero[-1]
            t_d = nt - int(np.argmin(zero[::-1])) if not zero.all() else 0          # first step of the zero tail
            assert np.all(zero[t_d:]) and (t_d == 0 or not zero[t_d - 1])
            # the state the trajectory had when it stopped is the one the host loop reports as final
            np.testing.assert_allclose(dev["x_all"][t_d, b], host["x_final"][b], atol=1e-8, rtol=0)
        assert np.all(np.any(dev["u_all"][:, live] != 0.0, axis=(0, 2)))
    finally:
        mpc._close()


# ------------------------------------------------------------------------------------------------ 8: X / U checks
def test_x_and_u_checks_count_like_their_numpy_twin(hip_lib):
    mpc, w = _cartpole(False)
    th, ga, dist = _draws(w)
    free = _session(mpc, _linear(w), P_LOSS, REF, th, ga, dist)
    # sets tighter than the trajectories: half the reached position range, half the largest input
    px, pu = 0.5 * np.abs(free["x_all"][:, :, 0]).max(), 0.5 * np.abs(free["u_all"]).max()
    HX = np.zeros((2, 4))
    HX[0, 0], HX[1, 0] = 1.0, -1.0
    X = Polytope(HX, np.array([px, px]))
    U = Polytope(np.array([[1.0], [-1.0]]), np.array([pu, pu]))
    dev = _session(mpc, _linear(w), P_LOSS, REF, th, ga, dist, X=X, U=U)
    assert dev["x_all"].tobytes() == free["x_all"].tobytes() and dev["u_all"].tobytes() == free["u_all"].tobytes()
    for key, H, hv, v in (("x_violations", HX, X.b, dev["x_all"]), ("u_violations", U.A, U.b, dev["u_all"])):
        m = np.einsum("ri,tbi->tbr", np.asarray(H, dtype=np.float64), v) - np.asarray(hv, dtype=np.float64).reshape(-1)
        assert np.abs(m - 1e-7).min() > 1e-9, (key, np.abs(m - 1e-7).min())       # no row sits on the threshold
        want = np.sum(np.any(m > 1e-7, axis=2), axis=0)
        assert np.any((want > 0) & (want < T)), (key, want)                        # some trajectory is out some of the time
        print(f"   {key}: {want.tolist()}")
        assert np.array_equal(dev[key], want), (key, dev[key], want)


# ------------------------------------------------------------------------------------------------ 9: lifecycle
def test_session_lifecycle(hip_lib):
    mpc, w = common.make_mpc("cartpole", 10, True, create=True)
    h = mpc._handle
    L = _native.lib()
    nb, nt = 8, 6
    p_loss = np.tile([0.0, 0.3, 0.6, 0.9], 2)
    th, ga, dist = _draws(w, nb, nt, seed=9)
    ref = 0.5 * np.ones(nt)
    before = mpc.run_closed_loop(p_loss, ref, th, ga, dist)
    ses = mpc.open_closed_loop(p_loss, ref, th, ga)
    x = np.zeros((nb, 4))
    u0 = ses.step(x).copy()
    # a second open, and everything that would re-carve the session's memory, is refused and leaves the session as it is
    rc, msg = raw_open(h, nb, nt)
    assert rc == E_INVALID and "already open" in msg
    with pytest.raises(RuntimeError, match="stepped closed loop is open"):
        mpc.determine_packets(np.zeros((nb, 4)), np.zeros((nb, 4)))                 # tmpc_solve_batch
    with pytest.raises(RuntimeError, match="stepped closed loop is open"):
        mpc.run_closed_loop(p_loss, ref, th, ga, dist)
    # so is every setter: the session was carved for the settings of its open (timing off here: no tick sums to add to), and a
    # refused loop call must not have changed one on its way to the refusal
    with pytest.raises(RuntimeError, match="stepped closed loop is open"):
        mpc.run_closed_loop(p_loss, ref, th, ga, dist, timing=True, warm_start=True, capture=1, fused="off")
    with pytest.raises(RuntimeError, match="stepped closed loop is open"):
        mpc.set_kernel_path("block")
    par = (ctypes.c_double * 7)(1, 0.1, 0, 0.001, 9.8, 0.5, 0.02)
    for call in (lambda: L.tmpc_set_solve_timing(h.ptr, 1), lambda: L.tmpc_set_kernel_path(h.ptr, 2), lambda: L.tmpc_set_call_overlap(h.ptr, 0),
                 lambda: L.tmpc_mc_set_actuator(h.ptr, 1), lambda: L.tmpc_mc_set_plant(h.ptr, 1, par, 10), lambda: L.tmpc_mc_set_capture(h.ptr, 2),
                 lambda: L.tmpc_mc_set_device_rng(h.ptr, 1, 5, 0, None), lambda: L.tmpc_mc_set_warm_start(h.ptr, 1),
                 lambda: L.tmpc_mc_set_fused(h.ptr, 0)):
        assert call() == E_INVALID and "stepped closed loop is open" in h.error()
    plant = _linear(w)
    us = [u0]
    x = plant(x, u0) + dist[:, 0]
    for t in range(1, nt):
        us.append(ses.step(x).copy())
        x = plant(x, us[-1]) + dist[:, t]
    u = np.zeros((nb, 1))
    assert L.tmpc_mc_step(h.ptr, x.ctypes.data, u.ctypes.data) == E_INVALID and "T steps" in h.error()      # step T + 1
    stats = ses.close()
    assert stats["steps"] == nt
    same = _session(mpc, plant, p_loss, ref, th, ga, dist)                          # the refused calls changed nothing:
    assert np.array(us).tobytes() == same["u_all"].tobytes()                        # not the steps that followed them,
    for k in ("err2", "tube_violations", "x_violations", "u_violations", "not_optimal", "consistent", "iters_sum"):
        assert same[k].tobytes() == stats[k].tobytes(), k                           # not the statistics,
    assert "solve_time_mean" not in stats and "x_traj" not in stats
    after = mpc.run_closed_loop(p_loss, ref, th, ga, dist)
    for k in ("err2", "tube_violations", "not_optimal", "x_final", "consistent", "iters_sum"):
        assert after[k].tobytes() == before[k].tobytes(), k                         # nor the handle's settings
    assert L.tmpc_mc_close(h.ptr, *([None] * 8)) == E_INVALID                       # closed is closed
    # a session opened WITH timing keeps it: switching it off under the session is refused too, and close has the times
    ses = mpc.open_closed_loop(p_loss, ref, th, ga, timing=True)
    u0 = ses.step(np.zeros((nb, 4)))
    assert L.tmpc_set_solve_timing(h.ptr, 0) == E_INVALID
    ses.step(plant(np.zeros((nb, 4)), u0) + dist[:, 0])
    timed = ses.close()
    assert timed["steps"] == 2 and np.all(timed["solve_time_mean"] > 0) and np.all(timed["solve_time_max"] >= timed["solve_time_mean"])
    # a handle destroyed with an open session: the next handle works
    ses = mpc.open_closed_loop(p_loss, ref, th, ga)
    ses.step(np.zeros((nb, 4)))
    mpc._close()
    mpc2, _ = common.make_mpc("cartpole", 10, True, create=True)
    try:
        again = mpc2.run_closed_loop(p_loss, ref, th, ga, dist)
        assert again["err2"].tobytes() == before["err2"].tobytes()
    finally:
        mpc2._close()


# ------------------------------------------------------------------------------------------------ 10: the example
def test_external_plant_example_runs(hip_lib):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([common.PKG, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.join(common.ROOT, "examples", "external_plant.py"), "--trajectories", "8", "--steps", "40"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "p_loss" in r.stdout and "tube" in r.stdout

