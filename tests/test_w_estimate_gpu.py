"""The disturbance-set estimation on the device (include/tmpc.h: tmpc_estimate_w, tmpc_order_statistics; csrc/tmpc_west.hip) against its
numpy twin (montecarlo.estimate_disturbance_box_host) and against numpy.partition of the device's own samples.

SAMPLE_TOL: the largest |samples_device - samples_twin| measured on the MI355X at 256 trajectories x 400 periods is MEASURED_GAP
(both ways of giving the initial states); the bound is 100 times that -- round-off varies with the inputs, the device
contracts to FMA and its sin / cos are not numpy's -- and stays below the 1e-10 tests/test_closed_loop.py allows device-versus-host
quantities of this plant."""
import numpy as np
import pytest

import w_cases
from LinearMPCOverNetworks import montecarlo

pytestmark = pytest.mark.gpu

MEASURED_GAP = 3.11e-15     # 3.108624e-15 with the reference-order initial states and with the device's own draws
SAMPLE_TOL = 100.0 * MEASURED_GAP
BOX = montecarlo.W_REFERENCE_X0_BOX


def test_the_bound_is_no_wider_than_the_closed_loop_tests_allow():
    assert 0.0 < SAMPLE_TOL <= 1e-10


@pytest.fixture(scope="module")
def model():
    return w_cases.scenario()


def _check_against_own_samples(out):
    """order statistics, minimum and maximum equal numpy's on the device's own copied-out samples"""
    flat = out["samples"].reshape(4, -1)
    for c in range(4):
        for r, g in zip(out["ranks"], out["order_stats"][c]):
            assert g == np.partition(flat[c], r)[r], (c, int(r))
        assert out["min"][c] == flat[c].min() and out["max"][c] == flat[c].max()


@pytest.mark.parametrize("drawn", [False, True])
def test_samples_and_box_against_the_twin(hip_lib, model, drawn):
    A, B, K = model
    n, T = 256, 400
    if drawn:
        x0 = montecarlo.draw_initial_states_philox(n, *BOX, seed=456, first=0)
        dev = montecarlo.estimate_disturbance_box(A, B, K, T=T, x0_box=BOX, n_traj=n, seed=456, want_samples=True)
    else:
        x0 = montecarlo.reference_initial_states(n, 456)
        dev = montecarlo.estimate_disturbance_box(A, B, K, x0=x0, T=T, want_samples=True)
    tw = montecarlo.estimate_disturbance_box_host(A, B, K, x0, T)
    assert np.array_equal(dev["x0_used"], x0)
    gap = float(np.max(np.abs(dev["samples"] - tw["samples"])))
    gap_box = float(max(np.max(np.abs(dev["lo"] - tw["lo"])), np.max(np.abs(dev["hi"] - tw["hi"]))))
    print(f"\n256 x 400, drawn = {drawn}: max |samples_dev - samples_twin| = {gap:.3e}, max |box_dev - box_twin| = {gap_box:.3e}, "
          f"rollout {dev['rollout_ms']:.3f} ms, selection {dev['selection_ms']:.3f} ms")
    assert dev["n_samples"] == tw["n_samples"] == n * (T - 1)
    assert np.all(dev["n_nonfinite"] == 0) and dev["not_settled"] == tw["not_settled"] == 0
    assert gap <= SAMPLE_TOL
    assert gap_box <= SAMPLE_TOL                           # order statistics are 1-Lipschitz in the sup norm of the samples
    assert np.max(np.abs(dev["min"] - tw["min"])) <= SAMPLE_TOL and np.max(np.abs(dev["max"] - tw["max"])) <= SAMPLE_TOL
    assert abs(dev["x_final_norm_max"] - tw["x_final_norm_max"]) <= SAMPLE_TOL
    assert np.array_equal(dev["w_bound"], np.maximum(np.abs(dev["lo"]), np.abs(dev["hi"])))


def test_selection_is_exact_on_the_devices_own_samples(hip_lib, model):
    A, B, K = model
    n, T = 256, 400
    ns = n * (T - 1)
    ranks = w_cases.ranks_for(ns)
    out = hip_lib.estimate_w(A, B, K, T, x0_box=BOX, n_traj=n, seed=456, ranks=ranks, want_samples=True)
    out["ranks"], out["min"], out["max"] = ranks, out["w_min"], out["w_max"]
    assert out["n_samples"] == ns and 0 in ranks and ns - 1 in ranks and ranks.size == 6
    _check_against_own_samples(out)
    # the same columns through the stand-alone export
    alone = hip_lib.order_statistics(out["samples"].reshape(4, -1).T, ranks)
    assert np.array_equal(alone["order_stats"], out["order_stats"]) and np.all(alone["n_nonfinite"] == 0)


def test_adversarial_columns_through_the_selection_export(hip_lib):
    for name, col in w_cases.selection_cases().items():
        n_valid = int((~np.isnan(col)).sum())
        ranks = w_cases.ranks_for(col.size, n_valid)
        out = hip_lib.order_statistics(col, ranks)
        w_cases.check_selection(col, out["order_stats"][0], out["n_nonfinite"][0], ranks)
    # several columns, more ranks than one group of eight, a rank beyond the values that are not NaN
    rng = np.random.default_rng(5)
    n = 70001
    data = np.stack([rng.standard_normal(n), rng.integers(0, 3, n) * 1.0, np.full(n, -0.0), rng.standard_normal(n) ** 3], axis=1)
    data[5, 3] = np.nan
    ranks = np.r_[rng.integers(0, n - 1, 17), 0, n - 1]
    out = hip_lib.order_statistics(data, ranks)
    for c in range(3):
        w_cases.check_selection(data[:, c], out["order_stats"][c], out["n_nonfinite"][c], ranks)
    w_cases.check_selection(data[:, 3], out["order_stats"][3][:-1], out["n_nonfinite"][3], ranks[:-1])
    assert np.isnan(out["order_stats"][3][-1])


def test_a_trajectory_does_not_depend_on_how_the_sweep_is_split(hip_lib, model):
    A, B, K = model
    T = 400
    whole = hip_lib.estimate_w(A, B, K, T, x0_box=BOX, n_traj=256, seed=9, first=0, want_samples=True)
    a = hip_lib.estimate_w(A, B, K, T, x0_box=BOX, n_traj=128, seed=9, first=0, want_samples=True)
    b = hip_lib.estimate_w(A, B, K, T, x0_box=BOX, n_traj=128, seed=9, first=128, want_samples=True)
    both = np.concatenate([a["samples"], b["samples"]], axis=2)
    assert np.array_equal(whole["samples"].view(np.uint64), both.view(np.uint64))
    assert np.array_equal(whole["x0_used"], np.concatenate([a["x0_used"], b["x0_used"]]))
    assert np.array_equal(whole["w_min"], np.minimum(a["w_min"], b["w_min"])) and np.array_equal(whole["w_max"], np.maximum(a["w_max"], b["w_max"]))


def test_full_size(hip_lib, model):
    """65 536 trajectories x 400 periods from the reference's box: 26 M samples per component, an 837 MB buffer on the device.
    Values and times are printed, not gated."""
    A, B, K = model
    out = montecarlo.estimate_disturbance_box(A, B, K, T=400, x0_box=BOX, n_traj=65536, seed=456)
    print(f"\n65536 x 400: lo {out['lo']}, hi {out['hi']}, min {out['min']}, max {out['max']}, max |x_T| {out['x_final_norm_max']:.3e}, "
          f"rollout {out['rollout_ms']:.2f} ms, selection {out['selection_ms']:.2f} ms")
    assert out["n_samples"] == 65536 * 399
    assert np.all(out["n_nonfinite"] == 0) and out["not_settled"] == 0
    for c in range(4):
        assert out["min"][c] <= out["lo"][c] < 0.0 < out["hi"][c] <= out["max"][c]


def test_error_paths_launch_nothing(hip_lib, model):
    A, B, K = model
    with pytest.raises(RuntimeError, match=r"tmpc_estimate_w failed \(-2\)"):          # TMPC_E_UNSUPPORTED
        hip_lib.estimate_w(A, B, K, 400, x0_box=BOX, n_traj=64, plant="linear")
    with pytest.raises(RuntimeError, match=r"tmpc_estimate_w failed \(-1\)"):          # TMPC_E_INVALID
        hip_lib.estimate_w(A, B, K, 400, x0_box=BOX, n_traj=64, ranks=[0, 64 * 399])
    with pytest.raises(RuntimeError, match=r"tmpc_estimate_w failed \(-1\)"):
        hip_lib.estimate_w(A, B, K, 400, x0_box=BOX, n_traj=64, ranks=[-1])
    with pytest.raises(RuntimeError, match=r"tmpc_estimate_w failed \(-1\)"):
        hip_lib.estimate_w(A, B, K, 1, x0_box=BOX, n_traj=64)
    with pytest.raises(RuntimeError, match=r"tmpc_order_statistics failed \(-1\)"):
        hip_lib.order_statistics(np.arange(5.0), [5])
    # (-1000: no device of that number -- an argument error is reported before the device is touched)
    with pytest.raises(RuntimeError, match=r"tmpc_estimate_w failed \(-2\)"):
        hip_lib.estimate_w(A, B, K, 400, x0_box=BOX, n_traj=64, plant="linear", device=-1000)
    with pytest.raises(RuntimeError, match=r"tmpc_estimate_w failed \(-1\)"):
        hip_lib.estimate_w(A, B, K, 400, x0_box=BOX, n_traj=64, ranks=[64 * 399], device=-1000)
