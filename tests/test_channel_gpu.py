"""The Gilbert-Elliott loss channel and the link statistics in the device loops (include/tmpc.h: tmpc_mc_set_channel,
tmpc_mc_get_link_stats; csrc/tmpc_mc_step.hpp).  Bands: the project's own for the device loop against the host loop
(tests/test_closed_loop.py::test_device_resident_loop_equals_host_loop: integers equal, tracking_error to 1e-10, final states to
1e-8); where the same arithmetic runs twice, bytes.

B = 70 trajectories (more than one workgroup of four waves, and no multiple of it), T = 40 steps, every trajectory with its own
channel: trajectory 0 is the Bernoulli channel of p = 0.3 (p_gb = 0), trajectory 1 loses every packet after step 0, trajectory 2
never loses one although it changes state."""
import os
import re
import runpy
import sys

import numpy as np
import pytest

import common
from LinearMPCOverNetworks import _native, montecarlo, workloads
from test_stepped_loop_api import E_INVALID

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB, T = 70, 40
BERNOULLI, ALL_LOST, NEVER_LOST = 0, 1, 2
LINK = ("lost_up", "lost_down", "max_gap", "overrun")
KEYS = ("err2", "tube_violations", "not_optimal", "x_final", "consistent", "iters_sum") + LINK
CAP = ("x_traj", "x_nom_traj", "u_traj")
SEED = {("cartpole", False): 23, ("cartpole", True): 23, ("double_integrator", False): 41}


def _channel(nb=NB):
    rng = np.random.default_rng(17)
    ch = dict(p_gb=rng.uniform(0.05, 0.5, nb), p_bg=rng.uniform(0.1, 0.9, nb), e_g=rng.uniform(0.0, 0.2, nb), e_b=rng.uniform(0.5, 1.0, nb))
    for b, par in ((BERNOULLI, (0.0, 0.5, 0.3, 0.9)), (ALL_LOST, (1.0, 0.0, 0.1, 1.0)), (NEVER_LOST, (0.4, 0.3, 0.0, 0.0))):
        for k, v in zip(("p_gb", "p_bg", "e_g", "e_b"), par):
            ch[k][b] = v
    return ch


CH = _channel()
_CASE = {}


def _same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def _case(name, extended):
    """Controller, realisations and the HOST loop (numpy state machines and the numpy channel around the device solver) of a
    workload, computed once: the cart-pole at N = 10, or the double integrator as workloads.make_controller sets it up."""
    key = (name, extended)
    if key not in _CASE:
        if name == "cartpole":
            mpc, w = common.make_mpc("cartpole", 10, True, extended=extended, create=True)
            ref = np.where(np.arange(T) < T // 2, 0.5, -0.3)
        else:
            mpc, w = workloads.make_controller("double_integrator", 10, fixed_initial_state=False)
            ref = np.where(np.arange(T) < T // 2, 2.0, -1.2)
        th, ga, dist = montecarlo.draw_realisations(NB, T, w["w_bound"], seed=SEED[key])
        c = dict(mpc=mpc, w=w, ref=ref, th=th, ga=ga, dist=dist, extended=extended)
        c["host"] = _host_loop(c, channel=CH, capture=ALL_LOST)
        # the seeds are chosen so that every solve of the host loop is optimal: the integer statistics below are then exact
        assert np.all(c["host"]["not_optimal"] == 0), (key, c["host"]["not_optimal"])
        _CASE[key] = c
    return _CASE[key]


def _host_loop(c, p_loss=None, **kw):
    mpc, w = c["mpc"], c["w"]
    return montecarlo.run_remote_tube_mpc(mpc.determine_packets, w["A"], w["B"], mpc.get_steady_state_controller_gain(),
                                          mpc.get_ancillary_controller_gain(), mpc._N, mpc._Z, p_loss, c["ref"], c["th"], c["ga"], c["dist"],
                                          extended=c["extended"], **kw)


def _run(c, p_loss=None, channel=CH, **kw):
    return c["mpc"].run_closed_loop(p_loss, c["ref"], c["th"], c["ga"], c["dist"], extended=c["extended"], channel=channel, **kw)


def _against_host(label, dev, host):
    fig = {k: float(np.max(np.abs(dev[k] - host[k]))) for k in ("x_final", "tracking_error")}
    print(f"   {label}: max |device - host loop|: " + ", ".join(f"{k} {v:.1e}" for k, v in fig.items()))
    assert np.array_equal(dev["not_optimal"], host["not_optimal"]) and np.array_equal(dev["tube_violations"], host["tube_violations"])
    assert fig["tracking_error"] <= 1e-10 and fig["x_final"] <= 1e-8, fig
    for k in LINK:
        assert dev[k].dtype == np.int32 and np.array_equal(dev[k], host[k]), (k, dev[k], host[k])


CASES = [("cartpole", False), ("cartpole", True), ("double_integrator", False)]


# ------------------------------------------------------------------------------------------------ 1: the host loop
@pytest.mark.parametrize("name,extended", CASES)
def test_device_loop_equals_the_host_loop(hip_lib, name, extended):
    c = _case(name, extended)
    dev = _run(c)
    _against_host(f"{name}, extended = {extended}", dev, c["host"])
    arr = montecarlo.channel_arrivals(CH, c["th"], c["ga"])
    assert np.array_equal(dev["lost_up"], (arr["theta"] == 0).sum(axis=1)) and np.array_equal(dev["lost_down"], (arr["gamma"] == 0).sum(axis=1))
    assert dev["lost_up"][NEVER_LOST] == 0 and dev["lost_down"][NEVER_LOST] == 0 and dev["max_gap"][NEVER_LOST] == 0
    assert arr["state_up"][NEVER_LOST].any()                     # it does visit B, whose loss probability is 0
    assert 0 < dev["lost_up"][3:].min() and dev["lost_up"][3:].max() < T - 1 and dev["overrun"].sum() > dev["overrun"][ALL_LOST]      # (the twin's figures for these draws)
    assert dev["link_stats"]["max_gap"] is dev["max_gap"]


# ------------------------------------------------------------------------------------------------ 2: the loop forms
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("name,extended", CASES)
def test_loop_forms_agree_bit_for_bit(hip_lib, name, extended, warm):
    """One launch per sweep (closed_loop_kernel) or per problem and step (closed_loop_step_kernel, the extended controller) against
    solve launches + mc_step_kernel."""
    c = _case(name, extended)
    off = _run(c, fused="off", warm_start=warm, capture=5)
    on = _run(c, fused="on", warm_start=warm, capture=5)
    assert off["loop_mode"] == 0 and on["loop_mode"] == (2 if extended else 1)
    _same(on, off, KEYS + CAP)
    if warm:
        _against_host(f"{name}, extended = {extended}, warm start", on, c["host"])


def test_block_path_agrees_with_the_wave_path(hip_lib):
    """The workgroup-per-QP kernel solves the same QPs by another route: the band of tests/test_stepped_loop.py's block-kernel case,
    i.e. the device-against-host one, against the wave-path device run and against the host loop; the link statistics do not
    depend on the solver at all."""
    mpc, w = common.make_mpc("cartpole", 10, True, create=True)
    try:
        c = dict(_case("cartpole", False), mpc=mpc)
        assert mpc.get_kernel_path() == "wave"
        wave = _run(c, fused="off")
        mpc.set_kernel_path("block")
        assert mpc.get_kernel_path() == "block"
        blk = _run(c)
        assert blk["loop_mode"] == 0 and wave["loop_mode"] == 0
        _against_host("block kernel against the wave kernel", blk, wave)
        _against_host("block kernel against the host loop", blk, c["host"])
    finally:
        mpc._close()


# ------------------------------------------------------------------------------------------------ 3: the device generator
@pytest.mark.parametrize("name,extended", CASES[:2])
def test_device_generator_with_a_channel(hip_lib, name, extended):
    c = _case(name, extended)
    mpc, w, seed, first = c["mpc"], c["w"], 4242, 1000
    th, ga, dist = montecarlo.draw_realisations_philox(NB, T, w["w_bound"], seed=seed, first=first)
    fed = mpc.run_closed_loop(None, c["ref"], th, ga, dist, extended=extended, channel=CH)
    drawn = mpc.run_closed_loop(None, c["ref"], extended=extended, channel=CH, device_rng=(seed, first, w["w_bound"]))
    _same(drawn, fed)
    arr = montecarlo.channel_arrivals(CH, th, ga)
    assert np.array_equal(drawn["lost_up"], (arr["theta"] == 0).sum(axis=1)) and np.array_equal(drawn["lost_down"], (arr["gamma"] == 0).sum(axis=1))
    # the batch in two calls: trajectories first .. first + 27 and first + 27 .. first + 70, each with its slice of the channel
    cut = 27
    parts = [mpc.run_closed_loop(None, c["ref"], extended=extended, channel={k: v[s] for k, v in CH.items()},
                                 device_rng=(seed, first + s.start, w["w_bound"]), fused="off")
             for s in (slice(0, cut), slice(cut, NB))]
    whole = mpc.run_closed_loop(None, c["ref"], extended=extended, channel=CH, device_rng=(seed, first, w["w_bound"]), fused="off")
    _same({k: np.concatenate([p[k] for p in parts]) for k in KEYS}, whole)


# ------------------------------------------------------------------------------------------------ 4: the degenerate channel
@pytest.mark.parametrize("fused", ["off", "on"])
@pytest.mark.parametrize("name,extended", CASES)
def test_degenerate_channel_is_the_bernoulli_model_bit_for_bit(hip_lib, name, extended, fused):
    c = _case(name, extended)
    p_loss = np.tile([0.0, 0.3, 0.6, 0.9, 1.0, 0.123456789, 0.5], NB // 7)
    legacy = _run(c, p_loss=p_loss, channel=None, fused=fused, capture=3)
    chan = _run(c, channel=dict(p_gb=0.0, p_bg=0.4, e_g=p_loss, e_b=0.7), fused=fused, capture=3)
    assert chan["loop_mode"] == legacy["loop_mode"]
    _same(chan, legacy, KEYS + CAP)
    assert legacy["lost_up"].max() == T - 1 and legacy["lost_up"][0] == 0
    # and the legacy call that follows is not under the earlier channel
    again = _run(c, p_loss=p_loss, channel=None, fused=fused, capture=3)
    _same(again, legacy, KEYS + CAP)


# ------------------------------------------------------------------------------------------------ 5: every packet lost
@pytest.mark.parametrize("name,extended", CASES)
def test_all_lost_trajectory_runs_on_the_terminal_law(hip_lib, name, extended):
    c = _case(name, extended)
    mpc, host = c["mpc"], c["host"]
    N = mpc._N
    dev = _run(c, capture=ALL_LOST)
    assert dev["max_gap"][ALL_LOST] == T - 1 and dev["overrun"][ALL_LOST] == T - N
    assert dev["lost_up"][ALL_LOST] == T - 1 and dev["lost_down"][ALL_LOST] == T - 1
    for k in CAP:                                                # the recorded trajectory against the host loop's
        err = float(np.max(np.abs(dev[k] - host[k])))
        assert err <= 1e-8, (k, err)
    # beyond step N - 1 the applied input is the terminal law on the nominal state plus the ancillary feedback:
    # u_t = U_0[N] - K x_nom_t - K_anc (x_t - x_nom_t), U_0[N] the terminal column of the only packet that arrived
    x0 = np.zeros((1, mpc._nx))
    r0 = np.zeros((1, mpc._nx))
    r0[0, 0] = c["ref"][0]
    U0 = mpc.determine_packets(x0, r0, np.ones(1, np.uint8))[0] if extended else mpc.determine_packets(x0, r0)[0]
    K, Ka = mpc.get_steady_state_controller_gain(), mpc.get_ancillary_controller_gain()
    x, xn, u = dev["x_traj"][N:], dev["x_nom_traj"][N:], dev["u_traj"][N:]
    law = U0[0, :, N][None, :] - xn @ K.T - (x - xn) @ Ka.T
    assert np.max(np.abs(u - law)) <= 1e-8, np.max(np.abs(u - law))
    assert np.max(np.abs(dev["u_traj"][1:N] - (U0[0, :, 1:N].T - (dev["x_traj"][1:N] - dev["x_nom_traj"][1:N]) @ Ka.T))) <= 1e-8


# ------------------------------------------------------------------------------------------------ 6: R-MPC
def test_stopped_rmpc_trajectories_stop_counting(hip_lib):
    """The comparator (TrackingMPC + plain smart actuator) in the scenario of tests/test_fused_closed_loop.py: a trajectory whose
    solve is infeasible stops there, and so do its link statistics."""
    mpc, w = workloads.make_controller("double_integrator", 10, tracking=True)
    try:
        nt = 60
        rng = np.random.default_rng(11)
        x0 = (rng.uniform(-1, 1, (96, 2)) * [7.6, 0.6])[:NB]
        th, ga, dist = montecarlo.draw_realisations(NB, nt, 3.0 * w["w_bound"], seed=5)
        ref = np.where(np.arange(nt) < 30, 6.0, -6.0)
        ch = _channel()
        host = montecarlo.run_remote_tracking_mpc(mpc.determine_packets, w["A"], w["B"], mpc.get_steady_state_controller_gain(), 10,
                                                  None, ref, th, ga, dist, x0=x0, channel=ch)
        arr = montecarlo.channel_arrivals(ch, th, ga)
        full = (arr["theta"] == 0).sum(axis=1)
        for fused in ("off", "on"):
            dev = mpc.run_closed_loop(None, ref, th, ga, dist, x0=x0, channel=ch, fused=fused)
            dead = np.isnan(dev["tracking_error"])
            assert np.array_equal(dead, host["infeasible"]) and 0 < dead.sum() < NB
            for k in LINK:
                assert np.array_equal(dev[k], host[k]), (fused, k)
            assert np.array_equal(dev["lost_up"][~dead], full[~dead])
            assert np.all(dev["lost_up"][dead] <= full[dead]) and np.any(dev["lost_up"][dead] < full[dead])
    finally:
        mpc._close()


# ------------------------------------------------------------------------------------------------ 7: the stepped session
@pytest.mark.parametrize("extended", [False, True])
def test_session_with_a_channel_equals_the_run(hip_lib, extended):
    c = _case("cartpole", extended)
    mpc, w = c["mpc"], c["w"]
    A, B = np.asarray(w["A"], dtype=np.float64), np.asarray(w["B"], dtype=np.float64)
    run = _run(c, fused="off")
    x = np.zeros((NB, mpc._nx))
    h, L = mpc._handle, _native.lib()
    one = np.full(NB, 0.5)
    with mpc.open_closed_loop(None, c["ref"], c["th"], c["ga"], extended=extended, channel=CH) as s:
        for t in range(T):
            if t == 7:           # no setter changes the channel under an open session, and the session goes on
                assert L.tmpc_mc_set_channel(h.ptr, NB, *[one.ctypes.data] * 4) == E_INVALID and "stepped closed loop is open" in h.error()
                assert L.tmpc_mc_set_channel(h.ptr, 0, None, None, None, None) == E_INVALID
            u = s.step(x)
            x = x @ A.T + u @ B.T + c["dist"][:, t]
    ses = dict(s.stats, x_final=x)
    assert ses["steps"] == T
    _against_host(f"session against tmpc_mc_run, extended = {extended}", ses, run)
    _against_host(f"session against the host loop, extended = {extended}", ses, c["host"])
    assert np.array_equal(_native.mc_get_channel(h, NB), montecarlo.gilbert_elliott_thresholds(**CH))      # still set, as opened


@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("fused", ["off", "on"])
def test_session_fed_a_recorded_channel_trajectory_repeats_the_run(hip_lib, extended, fused):
    """As tests/test_stepped_loop.py::test_session_fed_a_recorded_trajectory_repeats_the_run does for the Bernoulli model: trajectory
    c of a tmpc_mc_run under the channel, recorded, is fed to trajectory c of a session under the same channel step by step -- the
    same inputs, statistics and link statistics BYTE FOR BYTE (mc_session_kernel against mc_step_kernel and against the fused
    kernels), whatever the other trajectories do.  c: the all-lost trajectory, the never-lost one and two generic ones."""
    c = _case("cartpole", extended)
    mpc, w = c["mpc"], c["w"]
    A, B = np.asarray(w["A"], dtype=np.float64), np.asarray(w["B"], dtype=np.float64)
    for k in (ALL_LOST, NEVER_LOST, 7, 69):
        run = _run(c, fused=fused, capture=k)
        assert run["loop_mode"] == (0 if fused == "off" else (2 if extended else 1))
        x = np.zeros((NB, mpc._nx))
        us = []
        with mpc.open_closed_loop(None, c["ref"], c["th"], c["ga"], extended=extended, channel=CH) as s:
            for t in range(T):
                x[k] = run["x_traj"][t]
                u = s.step(x)
                us.append(u[k].copy())
                x = x @ A.T + u @ B.T + c["dist"][:, t]
        ses = s.stats
        assert np.array(us).tobytes() == run["u_traj"].tobytes(), (k, np.max(np.abs(np.array(us) - run["u_traj"])))
        for q in ("err2", "tube_violations", "not_optimal", "iters_sum") + LINK:
            assert ses[q][k:k + 1].tobytes() == run[q][k:k + 1].tobytes(), (k, q, ses[q][k], run[q][k])
    assert run["lost_up"][69] > 0 and run["max_gap"][7] > 0           # (generic: they do lose packets)


# ------------------------------------------------------------------------------------------------ 8: statistics of the legacy model
@pytest.mark.parametrize("name,extended", CASES[:2])
def test_link_statistics_of_the_bernoulli_model(hip_lib, name, extended):
    c = _case(name, extended)
    p_loss = np.tile([0.0, 0.3, 0.6, 0.9, 0.95], NB // 5)
    host = _host_loop(c, p_loss=p_loss)
    assert np.all(host["not_optimal"] == 0)
    for fused in ("off", "on"):
        dev = _run(c, p_loss=p_loss, channel=None, fused=fused)
        _against_host(f"{name}, extended = {extended}, Bernoulli, fused {fused}", dev, host)
    want = (c["th"] < p_loss[:, None])[:, 1:].sum(axis=1)
    assert np.array_equal(dev["lost_up"], want) and dev["overrun"].sum() > 0 and dev["max_gap"].max() >= 10


# ------------------------------------------------------------------------------------------------ 9: the example
def test_bursty_losses_example_runs(hip_lib, capsys, monkeypatch):
    from LinearMPCOverNetworks import polytope_lite as pl
    old = pl.set_lp_backend("hip")           # the examples use the package defaults
    monkeypatch.setattr(sys, "argv", ["bursty_losses.py", "--trajectories", "8", "--steps", "50"])
    try:
        runpy.run_path(os.path.join(ROOT, "examples", "bursty_losses.py"), run_name="__main__")
    finally:
        pl.set_lp_backend(old)
    out = capsys.readouterr().out
    assert "cart-pole, N = 10: 24 trajectories, 50 steps, stationary loss rate 0.50" in out and "solves not optimal 0" in out
    rows = re.findall(r"mean burst +([0-9.]+): packets lost ([0-9.]+), tracking error ([0-9.]+), steps outside the tube (\d+), max_gap (\d+) "
                      r"\(mean ([0-9.]+)\), overrun steps (\d+) in (\d+) trajectories", out)
    assert [float(r[0]) for r in rows] == [2.0, 3.0, 12.0]
    assert int(rows[2][4]) >= int(rows[0][4]) and int(rows[2][6]) > 0          # the long bursts outlast the buffer
