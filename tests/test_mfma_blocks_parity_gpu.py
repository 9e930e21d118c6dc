"""The wave kernel with sweep A's G'DG pass on 4 x 4 x 4 matrix blocks (csrc/tmpc_wave.hpp: gdg_blocks; Shape::MFMA_BLOCKS of
csrc/tmpc_kernels.hip) against the oracle and against the workgroup-per-QP kernel, whose pass still multiplies 16 x 16
tiles: the bench shape on the 600 fixture states plus one infeasible and one unconstrained instance."""
import os

import numpy as np
import pytest

import common
from oracle.oracle import Oracle

ATOL_U = 1e-8          # tests/test_hip_parity.py
ATOL_SS = 1e-9
S = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
OUT_KEYS = ("u_nom", "x_nom0", "xu_ss", "x_nom", "status", "iters")


@pytest.fixture(scope="module")
def bench_reference(oracle_lib):
    mpc, _ = common.make_mpc("cartpole", 10, True, create=False)
    X = np.r_[S[:, :4], [[0.0, 0.0, 0.2, 0.0], [0.5, 0.0, 0.0, 0.0]]]      # + infeasible, + unconstrained
    R = np.r_[S[:, 4:], [[0.5, 0, 0, 0.0], [0.5, 0, 0, 0.0]]]
    ref = Oracle(mpc._problem_dict()).solve(X, R)
    assert list(ref["status"][-2:]) == [2, 0] and np.all(ref["status"][:600] == 0)
    return X, R, ref


@pytest.mark.gpu
def test_bench_shape_against_the_oracle_and_the_block_kernel(hip_lib, bench_reference):
    X, R, ref = bench_reference
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True)
    assert hip_lib.kernel_name(mpc._handle) == "tmpc::solve_kernel<11,1,0,5,4,0,8>"
    out = mpc._solve(X, R)
    again = mpc._solve(X, R)
    mpc.set_kernel_path("block")
    blk = mpc._solve(X, R)
    ok = ref["status"] == 0
    err_u = np.max(np.abs(out["u_nom"][ok] - ref["u_nom"][ok]))
    err_ss = np.max(np.abs(out["xu_ss"][ok] - ref["xu_ss"][ok]))
    d_it = np.abs(out["iters"].astype(np.int64) - blk["iters"].astype(np.int64))
    print(f"max |u_nom - oracle| {err_u:.2e}, max |xu_ss - oracle| {err_ss:.2e}, mean iterations {out['iters'][:600].mean():.4f} "
          f"(oracle {ref['iters'][:600].mean():.4f}, block kernel {blk['iters'][:600].mean():.4f}), "
          f"instances whose count differs from the block kernel's {int((d_it > 0).sum())} (max {int(d_it.max())})")
    assert np.array_equal(out["status"], ref["status"])
    assert np.array_equal(blk["status"], ref["status"])
    assert err_u <= ATOL_U and err_ss <= ATOL_SS
    assert np.all(np.isnan(out["u_nom"][600])) and out["iters"][601] == 0
    assert abs(out["iters"][:600].mean() - ref["iters"][:600].mean()) < 2.0
    assert d_it.max() <= 1
    for k in OUT_KEYS:
        assert np.array_equal(out[k], again[k], equal_nan=True), k
