"""A plant per trajectory in the tracking loops on the device (include/tmpc.h: tmpc_mc_run_plants, tmpc_plant_step_device;
TubeTrackingMPC.run_closed_loop(plant=<PlantFamily>)).  Shapes and bands: those of tests/test_stepped_loop.py -- B = 19, T = 40, loss rates
0 / 0.3 / 0.9, the stepping reference; integers equal, tracking_error to 1e-10, final states to 1e-8 (its _compare) -- and bytes where the
same kernels run twice.  The kernel alone: the bounds of tests/test_tracking_plants.py."""
import os
import re
import runpy
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import common
from LinearMPCOverNetworks import _native, montecarlo
from test_plant_models import NOMINAL
from test_stepped_loop import NB, P_LOSS, REF, SEED, T, _cartpole, _compare, _draws, _host_loop
from test_stepped_loop_api import E_INVALID
from test_tracking_plants import CARTPOLE_ATOL, cartpole_inputs, linear_bound, linear_family

pytestmark = pytest.mark.gpu

PLANT_SEED, SPREAD = 3, 0.1        # tests/test_plant_models.py: the family of its host loops
PHYS_ATOL = 1e-10                  # tests/test_closed_loop.py:173: the physics-rate error, device loop against host loop
STATS = ("err2", "tube_violations", "x_violations", "u_violations", "not_optimal", "consistent", "iters_sum")
_SHARED = {}


def _family(nb=NB):
    return montecarlo.sample_cartpole(nb, SPREAD, PLANT_SEED)


def _nominal_run():
    """The device loop on the ONE nominal cart-pole, launch per step: computed once, shared, not modified."""
    if "nominal" not in _SHARED:
        mpc, w = _cartpole(False)
        th, ga, dist = _draws(w)
        _SHARED["nominal"] = mpc.run_closed_loop(P_LOSS, REF, th, ga, dist, plant="cartpole", fused="off")
    return _SHARED["nominal"]


# ------------------------------------------------------------------------------------------------ 1: the kernel alone
@pytest.mark.parametrize("nb", [1, 63, 64, 65, 130])
def test_cartpole_kernel_alone(hip_lib, nb):
    import torch
    fam = montecarlo.sample_cartpole(nb, 0.2, 5)
    x, u = cartpole_inputs(nb, 1)
    w = np.random.default_rng(2).uniform(-1e-2, 1e-2, (nb, 4))
    xd, ud, wd = (torch.as_tensor(a, device="cuda") for a in (x, u, w))
    for wt, exp in ((None, fam(x, u)), (wd, fam(x, u) + w)):
        got = _native.plant_step(fam, xd, ud, w=wt).cpu().numpy()
        print(f"   cart-pole kernel, B = {nb}, w {'given' if wt is not None else 'absent'}: max |device - numpy| = {np.max(np.abs(got - exp)):.2e}")
        np.testing.assert_allclose(got, exp, atol=CARTPOLE_ATOL, rtol=0)
    assert np.array_equal(xd.cpu().numpy(), x)                            # the input is not written
    with pytest.raises(RuntimeError, match="overlaps x"):
        _native.plant_step(fam, xd, ud, x_plus=xd)


@pytest.mark.parametrize("nb", [1, 65])
@pytest.mark.parametrize("nx,nu", [(1, 1), (3, 2), (16, 4)])
def test_linear_kernel_alone(hip_lib, nx, nu, nb):
    import torch
    fam = linear_family(nb, nx, nu, 10 * nx + nu)
    rng = np.random.default_rng(4)
    x, u, w = rng.uniform(-2, 2, (nb, nx)), rng.uniform(-2, 2, (nb, nu)), rng.uniform(-0.1, 0.1, (nb, nx))
    xd, ud, wd = (torch.as_tensor(a, device="cuda") for a in (x, u, w))
    for wt, wn in ((None, None), (wd, w)):
        got = _native.plant_step(fam, xd, ud, w=wt).cpu().numpy()
        exp = fam(x, u) if wn is None else fam(x, u) + wn
        bound = linear_bound(fam, x, u, wn)
        print(f"   linear kernel ({nx}, {nu}), B = {nb}: max |device - numpy| / bound = {np.max(np.abs(got - exp) / bound):.2f}")
        assert np.all(np.abs(got - exp) <= bound)


# ------------------------------------------------------------------------------------------------ 2: a family against the host loop
@pytest.mark.parametrize("extended", [False, True])
def test_cartpole_family_equals_the_host_loop(hip_lib, extended):
    mpc, w = _cartpole(extended)
    th, ga, dist = _draws(w)
    fam = _family()
    host = _host_loop(mpc, w, P_LOSS, REF, th, ga, dist, extended, plant=fam)
    dev = mpc.run_closed_loop(P_LOSS, REF, th, ga, dist, extended=extended, plant=fam)
    _compare(f"cart-pole family of spread {SPREAD}, extended = {extended}", dev, host)
    gap = float(np.max(np.abs(dev["tracking_error_physics"] - host["tracking_error_physics"])))
    print(f"   max |tracking_error_physics: device - host| = {gap:.1e}; not_optimal {dev['not_optimal'].tolist()}")
    assert gap <= PHYS_ATOL
    assert dev["fused"] is False and dev["loop_mode"] == 0 and np.all(dev["x_violations"] == 0) and np.all(dev["u_violations"] == 0)
    for k in ("lost_up", "lost_down", "max_gap", "overrun"):
        assert np.array_equal(dev[k], host[k]), k
    if not extended:
        diff = np.abs(dev["x_final"] - _nominal_run()["x_final"]).max(axis=1)
        print(f"   min over the trajectories of |x_final - x_final(nominal plant)| = {diff.min():.1e}")
        assert np.all(diff > 1e-6)                                        # every trajectory really ran on another plant


# ------------------------------------------------------------------------------------------------ 3: nominal rows
def test_nominal_rows_equal_the_loops_own_plants(hip_lib):
    mpc, w = _cartpole(False)
    th, ga, dist = _draws(w)
    own = _nominal_run()
    dev = mpc.run_closed_loop(P_LOSS, REF, th, ga, dist, plant=montecarlo.plant_family("cartpole", par=np.tile(NOMINAL, (NB, 1))))
    _compare("19 nominal cart-pole rows against plant = 'cartpole'", dev, own)
    np.testing.assert_allclose(dev["tracking_error_physics"], own["tracking_error_physics"], atol=PHYS_ATOL, rtol=0)
    lin = montecarlo.plant_family("linear", A=np.tile(w["A"], (NB, 1, 1)), B=np.tile(w["B"], (NB, 1, 1)))
    dev = mpc.run_closed_loop(P_LOSS, REF, th, ga, dist, plant=lin)
    _compare("19 nominal linear rows against the linear plant", dev, mpc.run_closed_loop(P_LOSS, REF, th, ga, dist))
    assert "tracking_error_physics" not in dev


# ------------------------------------------------------------------------------------------------ 4: bytes where the same kernels run
def test_entry_point_equals_a_session_driven_from_python(hip_lib):
    """tmpc_mc_run_plants on host arrays against mpc.open_closed_loop stepped from Python around plant_step, on the same arrays."""
    import torch
    mpc, w = _cartpole(True)
    th, ga, dist = _draws(w)
    fam = _family()
    c = 7
    run = mpc.run_closed_loop(P_LOSS, REF, th, ga, dist, extended=True, plant=fam, capture=c)
    on_dev = SimpleNamespace(kind=fam.kind, substeps=fam.substeps, models=torch.as_tensor(fam.models, device="cuda"))
    wd = torch.as_tensor(np.ascontiguousarray(dist.transpose(1, 0, 2)), device="cuda")
    x = [torch.zeros((NB, 4), dtype=torch.float64, device="cuda"), torch.empty((NB, 4), dtype=torch.float64, device="cuda")]
    with mpc.open_closed_loop(P_LOSS, REF, th, ga, extended=True, capture=c) as s:
        for t in range(T):
            _native.plant_step(on_dev, x[t & 1], s.step(x[t & 1]), w=wd[t], x_plus=x[(t + 1) & 1])
        torch.cuda.synchronize()
    ses = s.stats
    assert ses["steps"] == T
    for k in STATS + ("x_traj", "x_nom_traj", "u_traj"):
        assert run[k].tobytes() == ses[k].tobytes(), k
    assert run["x_final"].tobytes() == x[T & 1].cpu().numpy().tobytes()


def test_shards_and_repeats_under_the_device_generator(hip_lib):
    mpc, w = _cartpole(False)
    fam = _family()
    whole = mpc.run_closed_loop(P_LOSS, REF, plant=fam, device_rng=(SEED, 100, w["w_bound"]))
    again = mpc.run_closed_loop(P_LOSS, REF, plant=fam, device_rng=(SEED, 100, w["w_bound"]))
    part = mpc.run_closed_loop(P_LOSS[5:15], REF, plant=fam[5:15], device_rng=(SEED, 105, w["w_bound"]))
    for k in ("err2", "x_final", "iters_sum", "err2_physics"):
        assert part[k].tobytes() == np.ascontiguousarray(whole[k][5:15]).tobytes(), k
        assert again[k].tobytes() == whole[k].tobytes(), k
    # and the generator's numbers are the host twin's: the same loop on draw_realisations_philox's arrays
    thp, gap, distp = montecarlo.draw_realisations_philox(NB, T, w["w_bound"], seed=SEED, first=100)
    arrays = mpc.run_closed_loop(P_LOSS, REF, thp, gap, distp, plant=fam)
    for k in ("err2", "x_final", "iters_sum", "err2_physics", "not_optimal", "tube_violations"):
        assert arrays[k].tobytes() == whole[k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 5: a linear family with several inputs
def test_two_input_linear_family_equals_the_host_loop(hip_lib):
    from test_closed_loop_several_inputs import two_input_mpc
    mpc, w = two_input_mpc(False, device=0)
    try:
        nb, nt = 9, 30
        p_loss = np.tile([0.0, 0.3, 0.9], 3)
        th, ga, dist = _draws(w, nb, nt, seed=32)
        ref = np.where(np.arange(nt) < nt // 2, 2.0, -1.2)
        rng = np.random.default_rng(17)
        rel = rng.uniform(0.01, 0.03, (nb, 1, 1))                          # 1 - 3 % per trajectory, every entry its own sign and size
        fam = montecarlo.plant_family("linear", A=w["A"] * (1.0 + rel * rng.uniform(-1, 1, (nb, 3, 3))),
                                      B=w["B"] * (1.0 + rel * rng.uniform(-1, 1, (nb, 3, 2))))
        host = _host_loop(mpc, w, p_loss, ref, th, ga, dist, False, plant=fam)
        dev = mpc.run_closed_loop(p_loss, ref, th, ga, dist, plant=fam, capture=8)
        _compare("two inputs (nx 3, nu 2, N 5), perturbed linear family", dev, host)
        assert np.abs(dev["u_traj"][:, 1]).max() > 1e-3                    # the second input is in use
        nominal = mpc.run_closed_loop(p_loss, ref, th, ga, dist)
        assert np.all(np.abs(dev["x_final"] - nominal["x_final"]).max(axis=1) > 1e-6)
    finally:
        mpc._close()


# ------------------------------------------------------------------------------------------------ 6: R-MPC
def test_rmpc_on_a_family_stops_infeasible_trajectories(hip_lib):
    """The scenario of tests/test_stepped_loop.py::test_rmpc_session_stops_infeasible_trajectories_with_zero_input on a perturbed family."""
    from test_tracking_mpc import _make
    mpc, w = _make(True)
    try:
        nb, nt = 64, 60
        rng = np.random.default_rng(11)
        x0 = (rng.uniform(-1, 1, (96, 2)) * [7.6, 0.6])[:nb]
        p_loss = np.tile([0.0, 0.3, 0.6, 0.9], nb // 4)
        th, ga, dist = montecarlo.draw_realisations(nb, nt, 3.0 * w["w_bound"], seed=5)
        ref = np.where(np.arange(nt) < 30, 6.0, -6.0)
        prng = np.random.default_rng(19)
        fam = montecarlo.plant_family("linear", A=w["A"] * (1.0 + 0.02 * prng.uniform(-1, 1, (nb, 2, 2))), B=w["B"] * (1.0 + 0.02 * prng.uniform(-1, 1, (nb, 2, 1))))
        host = montecarlo.run_remote_tracking_mpc(mpc.determine_packets, w["A"], w["B"], mpc.get_steady_state_controller_gain(), 10,
                                                  p_loss, ref, th, ga, dist, x0=x0, plant=fam)
        dead_host = host["infeasible"]
        assert 0 < dead_host.sum() < nb
        late = [b for b in np.flatnonzero(dead_host)]
        c = int(late[-1])
        dev = mpc.run_closed_loop(p_loss, ref, th, ga, dist, x0=x0, plant=fam, capture=c)
        dead = np.isnan(dev["tracking_error"])
        assert np.array_equal(dead, dead_host) and np.array_equal(dev["not_optimal"], host["not_optimal"])
        assert np.all(dev["not_optimal"][dead] == 1) and np.all(np.isnan(dev["err2"][dead]))
        live = ~dead
        np.testing.assert_allclose(dev["tracking_error"][live], host["tracking_error"][live], atol=1e-10, rtol=0)
        # a stopped trajectory keeps the state of its last step (the host loop freezes it there), the others end where the host loop ends
        np.testing.assert_allclose(dev["x_final"], host["x_final"], atol=1e-8, rtol=0)
        for k in ("lost_up", "lost_down", "max_gap", "overrun"):
            assert np.array_equal(dev[k], host[k]), k
        # the captured trajectory stops: u = 0 from that step on (its rows of the record stay zero), and the step before it led to x_final
        zero = np.all(dev["u_traj"] == 0.0, axis=1)
        assert zero[-1]
        t_d = nt - int(np.argmin(zero[::-1])) if not zero.all() else 0
        assert np.all(zero[t_d:]) and np.all(dev["x_traj"][t_d:] == 0.0)
        if t_d > 0:
            last = fam[c](dev["x_traj"][t_d - 1:t_d], dev["u_traj"][t_d - 1:t_d])[0] + dist[c, t_d - 1]
            np.testing.assert_allclose(dev["x_final"][c], last, atol=1e-8, rtol=0)
    finally:
        mpc._close()


# ------------------------------------------------------------------------------------------------ 7: settings and refusals
def test_settings_are_honoured_and_left_alone(hip_lib):
    mpc, w = _cartpole(False)
    h = mpc._handle
    th, ga, dist = _draws(w)
    fam = _family()
    before = mpc.run_closed_loop(P_LOSS, REF, th, ga, dist)
    # the Gilbert-Elliott channel
    ch = montecarlo.burst_channel(P_LOSS, np.maximum(3.0, 1.0 / (1.0 - P_LOSS)))
    _compare("channel", mpc.run_closed_loop(None, REF, th, ga, dist, plant=fam, channel=ch), _host_loop(mpc, w, None, REF, th, ga, dist, False, plant=fam, channel=ch))
    # two full-state schedules shared by the batch
    tab = np.zeros((2, T, 4))
    tab[0, :, 0], tab[1, :, 0] = REF, -REF
    ids = np.arange(NB) % 2
    dev = mpc.run_closed_loop(P_LOSS, tab, th, ga, dist, plant=fam, ref_id=ids)
    host = _host_loop(mpc, w, P_LOSS, tab[ids], th, ga, dist, False, plant=fam)
    _compare("reference table, K = 2", dev, host)
    np.testing.assert_allclose(dev["tracking_error_physics"], host["tracking_error_physics"], atol=PHYS_ATOL, rtol=0)
    # warm start against the cold run
    cold = mpc.run_closed_loop(P_LOSS, REF, th, ga, dist, plant=fam)
    warm = mpc.run_closed_loop(P_LOSS, REF, th, ga, dist, plant=fam, warm_start=True)
    _compare("warm start against cold", warm, cold)
    print(f"   interior-point iterations: cold {cold['iters_sum'].sum()}, warm {warm['iters_sum'].sum()}")
    assert warm["iters_sum"].sum() < cold["iters_sum"].sum()
    # timing and capture come back as after a session
    timed = mpc.run_closed_loop(P_LOSS, REF, th, ga, dist, plant=fam, timing=True, capture=3)
    assert np.all(timed["solve_time_mean"] > 0) and timed["x_traj"].shape == (T, 4) and timed["err2"].tobytes() == cold["err2"].tobytes()
    # a batch that does not fit a channel that is set launches nothing
    L = _native.lib()
    assert _native.mc_set_channel(h, ch) == NB
    _native.kernel_ms_total(h, reset=True)
    _native.lane_counters(h, reset=True)
    rows = np.ascontiguousarray(fam.models[:8])
    z = np.zeros((8, T, 4))
    rc = L.tmpc_mc_run_plants(h.ptr, 8, T, 0, 1, rows.ctypes.data, 10, None, REF.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, None,
                              *([None, None, 0] * 3), *([None] * 9))
    assert rc == E_INVALID and h.error() == "tmpc_mc_run_plants: B = 8, but the loss channel was set for B = 19 trajectories"
    assert _native.kernel_ms_total(h)[1] == 0 and _native.lane_counters(h)[0] == (0, 0)
    _native.mc_set_channel(h, None)
    # the regulator loop's setter still refuses the tracking handle
    with pytest.raises(RuntimeError, match=r"failed \(-2\).*only regulator handles"):
        _native.mc_set_plant_models(h, "linear", np.zeros((4, 4, 5)))
    # and the loop without a family is what it was
    after = mpc.run_closed_loop(P_LOSS, REF, th, ga, dist)
    for k in ("err2", "tube_violations", "not_optimal", "x_final", "consistent", "iters_sum"):
        assert after[k].tobytes() == before[k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 8: the entry points
def test_sweep_on_the_device_equals_the_host_sweep(hip_lib):
    mpc, w = _cartpole(False)
    p_loss, n_mc, nt = np.array([0.0, 0.3, 0.6, 0.9]), 3, 40
    fam = montecarlo.sample_cartpole(len(p_loss) * n_mc, SPREAD, PLANT_SEED)
    dev, pi = montecarlo.mc_sweep(mpc, w, p_loss, n_mc, nt, 0.5, on_device=True, plant=fam, world=1)
    host, pi2 = montecarlo.mc_sweep(mpc, w, p_loss, n_mc, nt, 0.5, on_device=False, plant=fam, world=1)
    assert dev.shape == (12, 3) and np.array_equal(pi, pi2)
    np.testing.assert_allclose(dev[:, 0], host[:, 0], atol=1e-10, rtol=0)
    assert np.array_equal(dev[:, 1:], host[:, 1:])
    # the shard of a second rank is the slice of the family: the rows of the whole sweep, under the device generator
    lo, hi = montecarlo.shard_bounds(12, 1, 2)
    full, _ = montecarlo.mc_sweep(mpc, w, p_loss, n_mc, nt, 0.5, seed=77, on_device=True, plant=fam, world=1, device_rng=True)
    half = mpc.run_closed_loop(p_loss[pi[lo:hi]], np.full(nt, 0.5), plant=fam[lo:hi], device_rng=(77, lo, w["w_bound"]))
    assert half["tracking_error"].tobytes() == np.ascontiguousarray(full[lo:hi, 0]).tobytes()
    with pytest.raises(ValueError, match="holds 5 plants"):
        montecarlo.mc_sweep(mpc, w, p_loss, n_mc, nt, 0.5, on_device=True, plant=fam[:5])


def test_script_runs_with_a_plant_spread_on_the_device(hip_lib):
    r = subprocess.run([sys.executable, os.path.join(common.ROOT, "scripts", "mc_linear_system.py"), "--n-mc", "1", "--T", "20", "--N", "10",
                        "--plant-spread", "0.1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "== tube MPC, nonlinear cart-poles of spread 0.1: 10 trajectories x 20 steps" in r.stdout


def test_plant_uncertainty_example_runs_on_the_device(hip_lib, capsys, monkeypatch):
    """The assertions of tests/test_plant_models_gpu.py::test_plant_uncertainty_example_runs, and that step 3 went through the new entry point."""
    from LinearMPCOverNetworks import polytope_lite as pl
    calls = []
    real = _native.mc_run_plants
    monkeypatch.setattr(_native, "mc_run_plants", lambda *a, **k: calls.append(1) or real(*a, **k))
    old = pl.set_lp_backend("hip")           # the examples use the package defaults
    monkeypatch.setattr(sys, "argv", ["plant_uncertainty.py", "--trajectories", "16", "--steps", "50"])
    try:
        runpy.run_path(os.path.join(common.ROOT, "examples", "plant_uncertainty.py"), run_name="__main__")
    finally:
        pl.set_lp_backend(old)
    out = capsys.readouterr().out
    assert len(calls) == 2                                                # the two families; the nominal plant is the loop's own
    assert "cart-pole, N = 10: 16 trajectories per spread, 50 steps, loss rate 0.30" in out
    rows = re.findall(r"spread ([0-9.]+): tracking error ([0-9.]+) \(worst ([0-9.]+)\), tube_violations (\d+) in (\d+) trajectories, not_optimal (\d+)", out)
    assert [float(r[0]) for r in rows] == [0.0, 0.1, 0.2]
    assert all(0.0 < float(r[1]) < 0.2 for r in rows) and int(rows[0][5]) == int(rows[1][5]) == 0
