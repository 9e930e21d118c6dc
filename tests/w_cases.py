"""Inputs shared by tests/test_w_estimate.py (host execution model) and tests/test_w_estimate_gpu.py (device): the reference's
scenario of Results/estimate_W_for_Cartpole.py and adversarial columns for the selection kernels."""
import numpy as np

from LinearMPCOverNetworks import control_lite, montecarlo, workloads


def scenario():
    """(A, B, K) of estimate_W_for_Cartpole.py:20-58: the linearised cart-pole at 20 ms, the LQR gain for Q = diag(100, 10, 100, 10), R = 0.1"""
    m = workloads.cartpole()
    K, _, _ = control_lite.dlqr(m["A"], m["B"], m["Q"], m["R"])
    return m["A"], m["B"], np.asarray(K, dtype=np.float64).reshape(1, 4)


def ranks_for(n, n_valid=None):
    """ranks 0, n - 1 and the four quantile ranks of the 2.5 % discard (inside the ranked part of the column)"""
    m = n if n_valid is None else n_valid
    q, _ = montecarlo.quantile_ranks(m, 0.025)
    return np.unique(np.r_[0, m - 1, q])


def selection_cases():
    """name -> column.  Sizes from 1 to several workgroups' worth (a workgroup of the histogram kernel: 256 threads; a launch has one
    workgroup per 4096 values), none a multiple of 64 except where the case is about the size."""
    rng = np.random.default_rng(11)
    c = {}
    c["single"] = np.array([-3.5])
    c["two"] = np.array([2.0, -1.0])
    c["n63"] = rng.standard_normal(63)
    c["n65"] = rng.standard_normal(65)
    c["n257"] = rng.standard_normal(257) * 1e-6
    c["ties"] = rng.integers(-3, 4, 1001).astype(np.float64) * 1e-7            # seven distinct values
    c["settled"] = np.r_[rng.standard_normal(400) * 1e-5, np.full(613, 2.0 ** -60), np.full(500, -2.0 ** -61)]   # most values duplicates
    c["all_equal"] = np.full(777, 0.043)
    c["zeros_mixed"] = rng.permutation(np.r_[np.zeros(150), -np.zeros(151), [1e-300, -1e-300, 5e-324, -5e-324]])
    c["denormals"] = rng.permutation(np.r_[rng.integers(1, 1 << 40, 300).astype(np.uint64).view(np.float64),
                                           -rng.integers(1, 1 << 40, 301).astype(np.uint64).view(np.float64), [0.0, 2.3e-308]])
    c["negatives"] = -np.abs(rng.standard_normal(901)) - 1e-9
    c["inf"] = rng.permutation(np.r_[rng.standard_normal(500), [np.inf] * 3, [-np.inf] * 2, [1.7e308, -1.7e308]])
    c["nan"] = rng.permutation(np.r_[rng.standard_normal(700), [np.nan] * 5, [np.inf, -np.inf]])
    c["nan_payloads"] = rng.permutation(np.r_[rng.standard_normal(99), np.array([0x7ff0000000000001, 0xfff8000000000000, 0xffffffffffffffff],
                                                                               dtype=np.uint64).view(np.float64)])
    c["several_workgroups"] = rng.standard_normal(3 * 4096 + 37) * np.exp(rng.uniform(-30, 30, 3 * 4096 + 37))
    c["all_bit_patterns"] = rng.integers(0, 1 << 64, 2999, dtype=np.uint64).view(np.float64)       # a NaN or two among them
    return c


def check_selection(col, got, n_nonfinite, ranks):
    """got[r] == numpy.partition(col without NaN, r)[r], n_nonfinite exact"""
    col = np.asarray(col, dtype=np.float64)
    kept = col[~np.isnan(col)]
    assert n_nonfinite == int((~np.isfinite(col)).sum()), (n_nonfinite, int((~np.isfinite(col)).sum()))
    for r, g in zip(ranks, got):
        want = np.partition(kept, r)[r]
        assert g == want, (int(r), float(g), float(want))
