"""The disturbance set W estimated on the plant of the device closed loop: the numpy twin of the procedure of the
reference's Results/estimate_W_for_Cartpole.py on its own scenario, the initial-state draws, and the kernels' SOURCE
(csrc/tmpc_west.hip) on the host execution model of tests/wavesim under ASan + UBSan and under MSan.  CPU only."""
import importlib.util
import os
import sys

import numpy as np
import pytest

import common
import w_cases
from LinearMPCOverNetworks import montecarlo, workloads

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "wavesim"))
import hostsim  # noqa: E402
import west_case  # noqa: E402

SAN_ENV = hostsim.SAN_ENV
assert_clean = hostsim.assert_clean
BOX = montecarlo.W_REFERENCE_X0_BOX


@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    return hostsim.binaries_or_skip(tmp_path_factory, "westsim")


@pytest.fixture(scope="module")
def twin():
    A, B, K = w_cases.scenario()
    return montecarlo.estimate_disturbance_box_host(A, B, K, montecarlo.reference_initial_states(), 400)


# ---------------------------------------------------------------- initial states
def test_reference_initial_states_are_four_scalar_draws_per_trajectory():
    """estimate_W_for_Cartpole.py:82-85 draws position, velocity, angle and angular velocity one by one from default_rng(456)"""
    rng = np.random.default_rng(456)
    lo, hi = BOX
    want = np.array([[rng.uniform(lo[i], hi[i]) for i in range(4)] for _ in range(100)])
    assert np.array_equal(montecarlo.reference_initial_states(100, 456), want)
    assert np.array_equal(lo, [-1.0, -0.5, -0.3, -0.5]) and np.array_equal(hi, [1.0, 0.5, 0.3, 0.5])


def test_philox_initial_states_are_numpys_philox_words():
    """Key (seed, first + i), counter (0, 0, 0, 0): numpy.random.Philox increments its counter before it generates, so its counter
    starts one below -- at 2^64 - 1 in word 0, whose increment carries into word 1 (the convention tests/test_condense.py pins for
    montecarlo.philox4x64)."""
    lo, hi = BOX
    seed, first, n = 456, 7, 33
    got = montecarlo.draw_initial_states_philox(n, lo, hi, seed, first)
    for i in range(n):
        raw = np.random.Philox(key=[seed, first + i], counter=[2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1]).random_raw(4)
        u = (raw >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        assert np.array_equal(got[i], lo + (hi - lo) * u), i
    assert np.all(got >= lo) and np.all(got < hi)
    # a trajectory does not depend on how the sweep is split
    assert np.array_equal(got[10:], montecarlo.draw_initial_states_philox(n - 10, lo, hi, seed, first + 10))
    assert not np.array_equal(got, montecarlo.draw_initial_states_philox(n, lo, hi, seed + 1, first))


# ---------------------------------------------------------------- the numpy twin on the reference's scenario
def test_host_twin_on_the_reference_scenario(twin):
    """100 trajectories x 400 periods from default_rng(456)"""
    A, B, K = w_cases.scenario()
    assert twin["n_samples"] == 39900 and twin["samples"].shape == (4, 399, 100)
    assert twin["not_settled"] == 0 and twin["x_final_norm_max"] < 1e-3
    assert np.all(twin["n_nonfinite"] == 0)
    flat = twin["samples"].reshape(4, -1)
    for c in range(4):
        lo, hi = np.quantile(flat[c], [0.0125, 0.9875])
        assert twin["lo"][c] == lo and twin["hi"][c] == hi
        assert twin["min"][c] == flat[c].min() and twin["max"][c] == flat[c].max()
        assert twin["min"][c] <= twin["lo"][c] < 0.0 < twin["hi"][c] <= twin["max"][c]
    assert np.array_equal(twin["w_bound"], np.maximum(np.abs(twin["lo"]), np.abs(twin["hi"])))
    # the four order statistics the device is asked for reproduce numpy's quantiles through numpy's interpolation
    ranks, gam = montecarlo.quantile_ranks(39900, 0.025)
    for c in range(4):
        s = np.sort(flat[c])[ranks]
        assert montecarlo._lerp(s[0], s[1], gam[0]) == twin["lo"][c] and montecarlo._lerp(s[2], s[3], gam[1]) == twin["hi"][c]


def test_every_sample_is_the_one_step_prediction_error(twin):
    """x_{k+1} == Acl x_k + w_k with the states recomputed with workloads.cartpole_step -- as w_k == x_{k+1} - Acl x_k, the form that is
    exact in floating point (adding the rounded difference back need not return x_{k+1} to the last bit)"""
    A, B, K = w_cases.scenario()
    Acl = A - B @ K
    x = montecarlo.reference_initial_states()
    for k in range(399):
        u = ((-(K[0, 0] * x[:, 0]) - K[0, 1] * x[:, 1]) - K[0, 2] * x[:, 2]) - K[0, 3] * x[:, 3]
        xn = workloads.cartpole_step(x, u)
        pred = np.stack([((Acl[c, 0] * x[:, 0] + Acl[c, 1] * x[:, 1]) + Acl[c, 2] * x[:, 2]) + Acl[c, 3] * x[:, 3] for c in range(4)], axis=1)
        assert np.array_equal(twin["samples"][:, k, :].T, xn - pred), k
        assert np.max(np.abs(xn - (pred + twin["samples"][:, k, :].T))) <= 2.0 ** -52 * np.max(np.abs(xn)), k
        x = xn


def test_quantile_ranks_follow_numpys_linear_rule():
    rng = np.random.default_rng(2)
    for n in (1, 2, 7, 80, 81, 39900, 102144):
        col = rng.standard_normal(n)
        for discard in (0.025, 0.1, 0.5):
            ranks, gam = montecarlo.quantile_ranks(n, discard)
            s = np.sort(col)[ranks]
            lo, hi = np.quantile(col, [discard / 2, 1 - discard / 2])
            assert montecarlo._lerp(s[0], s[1], gam[0]) == lo and montecarlo._lerp(s[2], s[3], gam[1]) == hi, (n, discard)


# ---------------------------------------------------------------- the kernels' source on the host execution model
@pytest.mark.parametrize("build", ["westsim_asan", "westsim_msan"])
def test_selection_kernels_on_the_host_model(binaries, build):
    """Exact: == numpy.partition(col, r)[r] at ranks 0, n - 1 and the four quantile ranks (NaN left out and counted)."""
    for name, col in w_cases.selection_cases().items():
        n_valid = int((~np.isnan(col)).sum())
        ranks = w_cases.ranks_for(col.size, n_valid)
        out = west_case.run_select(binaries[build], col, ranks, env=SAN_ENV)
        assert_clean(out["stderr"])
        w_cases.check_selection(col, out["order_stats"][0], out["n_nonfinite"][0], ranks)


def test_selection_of_several_columns_and_more_ranks_than_one_group(binaries):
    """four columns side by side, 19 ranks (three groups of at most eight), a rank beyond the values that are not NaN"""
    rng = np.random.default_rng(5)
    n = 1500
    data = np.stack([rng.standard_normal(n), rng.integers(0, 3, n) * 1.0, np.full(n, -0.0), rng.standard_normal(n) ** 3], axis=1)
    data[5, 3] = np.nan
    ranks = np.r_[rng.integers(0, n - 1, 17), 0, n - 1]
    for build in ("westsim_asan", "westsim_msan"):
        out = west_case.run_select(binaries[build], data, ranks, env=SAN_ENV)
        assert_clean(out["stderr"])
        for c in range(3):
            w_cases.check_selection(data[:, c], out["order_stats"][c], out["n_nonfinite"][c], ranks)
        w_cases.check_selection(data[:, 3], out["order_stats"][3][:-1], out["n_nonfinite"][3], ranks[:-1])
        assert np.isnan(out["order_stats"][3][-1])        # rank n - 1 of n - 1 ranked values


@pytest.mark.parametrize("build", ["westsim_asan", "westsim_msan"])
def test_rollout_kernel_on_the_host_model(binaries, build):
    """64 trajectories x 50 periods against the numpy twin: the x86 build does not contract to FMA, only libm's sin / cos could differ"""
    A, B, K = w_cases.scenario()
    P = workloads.CARTPOLE_PARAMS
    par = [P["M"], P["m"], P["b"], P["I"], P["g"], P["l"], 0.02]
    x0 = montecarlo.draw_initial_states_philox(64, *BOX, seed=456, first=3)
    tw = montecarlo.estimate_disturbance_box_host(A, B, K, x0, 50)
    for kw in (dict(x0=x0), dict(box=BOX, n_traj=64, seed=456, first=3)):
        out = west_case.run_rollout(binaries[build], A - B @ K, K, par, 50, env=SAN_ENV, **kw)
        assert_clean(out["stderr"])
        assert np.array_equal(out["x0_used"], x0)
        np.testing.assert_allclose(out["samples"], tw["samples"], atol=1e-12, rtol=0)
        np.testing.assert_allclose(out["min"], tw["min"], atol=1e-12, rtol=0)
        np.testing.assert_allclose(out["max"], tw["max"], atol=1e-12, rtol=0)
        assert np.array_equal(out["min"], out["samples"].reshape(4, -1).min(axis=1))
        assert np.array_equal(out["max"], out["samples"].reshape(4, -1).max(axis=1))
        assert abs(np.max(out["xnorm"]) - tw["x_final_norm_max"]) <= 1e-12
    # a workgroup that is not full, and a second one
    out = west_case.run_rollout(binaries[build], A - B @ K, K, par, 4, x0=x0[:3], env=SAN_ENV)
    assert_clean(out["stderr"])
    np.testing.assert_allclose(out["samples"], montecarlo.estimate_disturbance_box_host(A, B, K, x0[:3], 4)["samples"], atol=1e-12, rtol=0)
    x0b = montecarlo.draw_initial_states_philox(70, *BOX, seed=1, first=0)
    out = west_case.run_rollout(binaries[build], A - B @ K, K, par, 3, box=BOX, n_traj=70, seed=1, env=SAN_ENV)
    assert_clean(out["stderr"])
    assert np.array_equal(out["x0_used"], x0b)
    np.testing.assert_allclose(out["samples"], montecarlo.estimate_disturbance_box_host(A, B, K, x0b, 3)["samples"], atol=1e-12, rtol=0)


# ---------------------------------------------------------------- the code object
def test_new_kernels_use_no_scratch_and_keep_clear_of_the_counted_names():
    spec = importlib.util.spec_from_file_location("code_object_notes", os.path.join(os.path.dirname(common.PKG), "scripts", "code_object_notes.py"))
    notes = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(notes)
    ks = notes.kernels(os.path.join(common.PKG, "lib", "libtmpc_hip.so"))
    dm = notes.demangle(list(ks))
    west = {dm[n]: k for n, k in ks.items() if "west_" in dm[n]}
    assert len(west) == 4 and all(any(t in n for n in west) for t in ("west_rollout_kernel", "west_hist_kernel", "west_narrow_kernel", "west_select_init_kernel")), sorted(west)
    for n, k in west.items():
        assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0, (n, k[".private_segment_fixed_size"], k[".vgpr_spill_count"])
        for counted in ("solve_kernel<", "closed_loop_kernel<", "closed_loop_step_kernel<", "solve_block_kernel<", "mc_step_kernel", "lp_kernel<"):
            assert counted not in n, n
