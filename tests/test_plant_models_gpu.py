"""A plant model per trajectory in the regulators' device loop and in the W estimate (include/tmpc.h: tmpc_mc_set_plant_models,
tmpc_estimate_w_models; csrc/tmpc_reg.hip, tmpc_west.hip).  Bands: the project's own for the regulator loops
(regulator_problems.compare_loops) and for the W estimate (tests/test_w_estimate_gpu.py: SAMPLE_TOL); where the same arithmetic runs
twice, bytes.  B = 70 trajectories: more than one workgroup of four waves, and no multiple of it."""
import os
import re
import runpy
import sys

import numpy as np
import pytest

import common  # noqa: F401  (sys.path)
import regulator_problems as rp
import w_cases
from LinearMPCOverNetworks import _native, montecarlo, workloads
from test_closed_loop_several_inputs import _regulator
from test_stepped_loop_api import E_INVALID
from test_w_estimate_gpu import SAMPLE_TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = ("x_traj", "x_nom_traj", "u_traj")
P = workloads.CARTPOLE_PARAMS
NOMINAL = np.array([P["M"], P["m"], P["b"], P["I"], P["g"], P["l"], 0.02])


def _same(a, b, keys, rows=slice(None), rows_b=slice(None)):
    for k in keys:
        assert np.asarray(a[k])[rows].tobytes() == np.asarray(b[k])[rows_b].tobytes(), k


# ------------------------------------------------------------------------------------------------ identity
def _regulator_case(tube):
    m, w = _regulator(tube)
    nb, steps = 70, 15
    rng = np.random.default_rng(9)
    x0 = rng.uniform(-1.0, 1.0, (nb, 3)) * [4.6, 3.0, 3.0]               # some start outside X: they fail at step 0
    x0[0] = [1.0, -0.5, 0.8]
    dist = rng.uniform(-1.0, 1.0, (nb, steps, 3)) * w["w_bound"]
    return m, w, nb, steps, x0, dist


@pytest.mark.parametrize("tube", [False, True])
def test_regulator_nominal_models_reproduce_the_run_without_models(hip_lib, tube):
    m, w, nb, steps, x0, dist = _regulator_case(tube)
    try:
        nominal = montecarlo.plant_family("linear", A=np.tile(w["A"], (nb, 1, 1)), B=np.tile(w["B"], (nb, 1, 1)))
        plain = m.run_closed_loop(x0, steps, w=dist, capture=0)
        with_models = m.run_closed_loop(x0, steps, w=dist, capture=0, plant=nominal)
        keys = ("cost", "x_viol", "u_viol", "tube_viol", "not_optimal", "fail_step", "x_final", "iters_sum") + CAP
        _same(with_models, plain, keys)
        _same(m.run_closed_loop(x0, steps, w=dist, capture=0), plain, keys)
        with pytest.raises(ValueError, match="linear plant family"):
            m.run_closed_loop(x0[:4], steps, plant=montecarlo.sample_cartpole(4, 0.1, 1))
    finally:
        m._close()


# ------------------------------------------------------------------------------------------------ regulators, nx = 3, nu = 2
def _regulator_host_loop(m, x0, w, sets, K, plant):
    """regulator_problems.host_loop with the plant line on the trajectory's own (A_b, B_b): numpy around per-step batch solves."""
    B, steps, nx = w.shape
    x = x0.copy()
    res = dict(cost=np.zeros(B), x_viol=np.zeros(B, np.int32), u_viol=np.zeros(B, np.int32), tube_viol=np.zeros(B, np.int32),
               not_optimal=np.zeros(B, np.int32), fail_step=np.full(B, -1, np.int32), iters_sum=np.zeros(B, np.int32))
    xs, xns, us = [x[0].copy()], [], []
    viol = lambda Pt, v: np.any(v @ Pt.A.T - Pt.b > 1e-7, axis=1)      # noqa: E731
    for t in range(steps):
        out = _native.solve_regulator_batch(m._handle, np.ascontiguousarray(x), want_traj=False)
        alive = res["fail_step"] < 0
        st = out["status"]
        res["iters_sum"] += np.where(alive, out["iters"], 0)
        res["not_optimal"] += (alive & (st != 0))
        newly = alive & (st >= 2)
        res["fail_step"][newly] = t
        go = alive & ~newly
        xn = out["x_nom0"]
        u = out["u_nom"][:, 0, :] - ((x - xn) @ K.T if K is not None else 0.0)
        res["cost"] += np.where(go, np.einsum("bi,ij,bj->b", x, m._Q, x) + np.einsum("bi,ij,bj->b", u, m._R, u), 0.0)
        for key, Pt, v in (("x_viol", sets.get("X"), x), ("u_viol", sets.get("U"), u), ("tube_viol", sets.get("Z"), x - xn)):
            if Pt is not None:
                res[key] += go & viol(Pt, v)
        x = np.where(go[:, None], plant(x, u) + w[:, t], x)
        xs.append(x[0].copy()); xns.append(xn[0].copy()); us.append(u[0].copy())      # noqa: E702
    res["x_final"] = x
    res["x_traj"], res["x_nom_traj"], res["u_traj"] = np.array(xs), np.array(xns), np.array(us)
    return res


@pytest.mark.parametrize("tube", [False, True])
def test_regulator_loop_with_a_plant_per_trajectory(hip_lib, tube):
    m, w, nb, steps, x0, dist = _regulator_case(tube)
    try:
        rng = np.random.default_rng(21)
        fam = montecarlo.plant_family("linear", A=w["A"][None] + 0.03 * rng.standard_normal((nb, 3, 3)), B=w["B"][None] + 0.05 * rng.standard_normal((nb, 3, 2)))
        sets = {"X": m._X, "U": m._U, "Z": m._Z} if tube else {"X": m._X, "U": m._U}
        K = m.get_controller_gain() if tube else None
        dev = m.run_closed_loop(x0, steps, w=dist, capture=0, plant=fam)
        host = _regulator_host_loop(m, x0, dist, sets, K, fam)
        n_fail = int(np.sum(host["fail_step"] >= 0))
        print(f"   regulator nx 3, nu 2, tube = {tube}, a plant per trajectory: {n_fail} of {nb} trajectories fail, "
              f"max |x_final(device) - x_final(host)| {float(np.max(np.abs(dev['x_final'] - host['x_final']))):.1e}")
        assert 0 < n_fail < nb
        rp.compare_loops(dev, host)
        plain = m.run_closed_loop(x0, steps, w=dist)
        alive = (host["fail_step"] < 0) & (plain["fail_step"] < 0)
        assert np.abs(dev["x_final"] - plain["x_final"])[alive].max(axis=1).min() > 1e-6       # every plant differs from the model
        # the device generator, and a shard of the batch on its own
        _, _, wp = montecarlo.draw_realisations_philox(nb, steps, w["w_bound"], seed=77, first=1000)
        dev = m.run_closed_loop(x0, steps, seed=77, first_trajectory=1000, w_bound=w["w_bound"], capture=0, plant=fam)
        rp.compare_loops(dev, _regulator_host_loop(m, x0, wp, sets, K, fam))
        part = m.run_closed_loop(x0[10:30], steps, seed=77, first_trajectory=1010, w_bound=w["w_bound"], plant=fam[10:30])
        _same(part, dev, ("cost", "x_final", "fail_step", "iters_sum"), rows_b=slice(10, 30))
    finally:
        m._close()


# ------------------------------------------------------------------------------------------------ the W estimate
def _west_same(a, b, cols=slice(None), cols_b=slice(None)):
    assert a["samples"][:, :, cols].tobytes() == b["samples"][:, :, cols_b].tobytes()
    assert a["x0_used"][cols].tobytes() == b["x0_used"][cols_b].tobytes()


def test_w_estimate_with_a_plant_per_trajectory(hip_lib):
    A, B, K = w_cases.scenario()
    n, steps = 70, 60
    box = montecarlo.W_REFERENCE_X0_BOX
    ranks = w_cases.ranks_for(n * (steps - 1))
    kw = dict(x0_box=box, n_traj=n, seed=456, first=3, ranks=ranks, want_samples=True)
    plain = hip_lib.estimate_w(A, B, K, steps, **kw)
    same = hip_lib.estimate_w(A, B, K, steps, par=np.tile(NOMINAL, (n, 1)), **kw)
    _west_same(same, plain)
    for k in ("order_stats", "w_min", "w_max", "n_nonfinite"):
        assert np.asarray(same[k]).tobytes() == np.asarray(plain[k]).tobytes(), k
    assert (same["n_samples"], same["not_settled"], same["x_final_norm_max"]) == (plain["n_samples"], plain["not_settled"], plain["x_final_norm_max"])
    fam = montecarlo.sample_cartpole(n, 0.2, 5)
    out = hip_lib.estimate_w(A, B, K, steps, par=fam.models, **kw)
    x0 = out["x0_used"]
    for b in (0, 41, 69):                                                # trajectory b alone: its plant, its initial state
        alone = hip_lib.estimate_w(A, B, K, steps, x0=x0[b:b + 1], par=fam.models[b:b + 1], want_samples=True)
        _west_same(alone, out, cols_b=slice(b, b + 1))
    flat = out["samples"].reshape(4, -1)
    for c in range(4):
        for r, g in zip(ranks, out["order_stats"][c]):
            assert g == np.partition(flat[c], r)[r], (c, int(r))
        assert out["w_min"][c] == flat[c].min() and out["w_max"][c] == flat[c].max()
    # against the numpy twin, through the public function
    dev = montecarlo.estimate_disturbance_box(A, B, K, T=steps, x0_box=box, n_traj=n, seed=456, first=3, want_samples=True, par=fam)
    tw = montecarlo.estimate_disturbance_box_host(A, B, K, x0, steps, par=fam)
    gap = float(np.max(np.abs(dev["samples"] - tw["samples"])))
    gap_box = float(max(np.max(np.abs(dev["lo"] - tw["lo"])), np.max(np.abs(dev["hi"] - tw["hi"]))))
    print(f"\n{n} x {steps}, a plant per trajectory: max |samples_dev - samples_twin| = {gap:.3e}, max |box_dev - box_twin| = {gap_box:.3e}")
    assert dev["samples"].tobytes() == out["samples"].tobytes() and dev["n_samples"] == tw["n_samples"] == n * (steps - 1)
    assert gap <= SAMPLE_TOL and gap_box <= SAMPLE_TOL
    assert np.max(np.abs(dev["min"] - tw["min"])) <= SAMPLE_TOL and np.max(np.abs(dev["max"] - tw["max"])) <= SAMPLE_TOL
    assert np.abs(out["samples"]).max() > 1.5 * np.abs(plain["samples"]).max()         # the mismatch is in the samples


# ------------------------------------------------------------------------------------------------ errors
def test_a_batch_that_does_not_fit_the_models_launches_nothing(hip_lib):
    m, w, nb, steps, x0, dist = _regulator_case(False)
    try:
        h = m._handle
        assert _native.mc_set_plant_models(h, "linear", montecarlo.plant_family("linear", A=np.tile(w["A"], (nb, 1, 1)), B=np.tile(w["B"], (nb, 1, 1))).models) == nb
        _native.kernel_ms_total(h, reset=True)
        _native.lane_counters(h, reset=True)
        x8 = np.ascontiguousarray(x0[:8])
        rc = _native.lib().tmpc_reg_run(h.ptr, 8, steps, x8.ctypes.data, None, None, None, 0, None, None, 0, None, None, 0, *([None] * 8), -1, None, None, None)
        assert rc == E_INVALID and h.error() == "tmpc_reg_run: B = 8, but the plant models were set for B = 70 trajectories"
        assert _native.kernel_ms_total(h)[1] == 0 and _native.lane_counters(h)[0] == (0, 0)
        assert np.all(np.isfinite(m.run_closed_loop(x0[:8], steps)["x_final"]))          # plant=None clears them: the handle runs any batch again
    finally:
        m._close()
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True)
    try:
        with pytest.raises(RuntimeError, match=r"failed \(-2\).*only regulator handles"):        # TMPC_E_UNSUPPORTED
            _native.mc_set_plant_models(mpc._handle, "linear", np.zeros((4, 4, 5)))
    finally:
        mpc._close()


# ------------------------------------------------------------------------------------------------ the example
def test_plant_uncertainty_example_runs(hip_lib, capsys, monkeypatch):
    from LinearMPCOverNetworks import polytope_lite as pl
    old = pl.set_lp_backend("hip")           # the examples use the package defaults
    monkeypatch.setattr(sys, "argv", ["plant_uncertainty.py", "--trajectories", "16", "--steps", "50"])
    try:
        runpy.run_path(os.path.join(ROOT, "examples", "plant_uncertainty.py"), run_name="__main__")
    finally:
        pl.set_lp_backend(old)
    out = capsys.readouterr().out
    assert "cart-pole, N = 10: 16 trajectories per spread, 50 steps, loss rate 0.30" in out
    assert len(re.findall(r"estimated on 256 plants of spread ([0-9.]+)", out)) == 2
    rows = re.findall(r"spread ([0-9.]+): tracking error ([0-9.]+) \(worst ([0-9.]+)\), tube_violations (\d+) in (\d+) trajectories, not_optimal (\d+)", out)
    assert [float(r[0]) for r in rows] == [0.0, 0.1, 0.2]
    assert all(0.0 < float(r[1]) < 0.2 for r in rows) and int(rows[0][5]) == int(rows[1][5]) == 0
