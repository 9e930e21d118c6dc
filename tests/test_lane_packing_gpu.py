"""Lane packing on the device (csrc/tmpc_api.cpp: upload_wave): handles laid out packed (the default) and with
TMPC_NO_LANE_PACKING=1, read at tmpc_create.  A packed handle runs the same kernel on another layout -- 14 terminal-set functionals of
the bench problem as dense rows, one factored slot skipped -- so its answers are the oracle's to the parity tolerance, not the unpacked
handle's bit for bit; a problem that does not pack must not notice the change at all."""
import os

import numpy as np
import pytest

import common
import shape_cases
from LinearMPCOverNetworks import _native, montecarlo
from LinearMPCOverNetworks.polytope_lite import Polytope
from oracle.oracle import Oracle

ATOL_U = 1e-8          # tests/test_hip_parity.py
S = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
OUT_KEYS = ("u_nom", "x_nom0", "xu_ss", "x_nom", "status", "iters")


def _make(monkeypatch, packed, *args, **kw):
    """common.make_mpc with its device problem, laid out packed or not (the variable is read by tmpc_create only)"""
    if packed:
        monkeypatch.delenv("TMPC_NO_LANE_PACKING", raising=False)
    else:
        monkeypatch.setenv("TMPC_NO_LANE_PACKING", "1")
    mpc, w = common.make_mpc(*args, create=True, **kw)
    monkeypatch.delenv("TMPC_NO_LANE_PACKING", raising=False)
    return mpc, w


@pytest.fixture(scope="module")
def bench_reference(oracle_lib):
    """the 600 fixture states and the two edge cases of tests/test_residual_scale_gpu.py, with the oracle's answers"""
    mpc, _ = common.make_mpc("cartpole", 10, True, create=False)
    X = np.r_[S[:, :4], [[0.0, 0.0, 0.2, 0.0], [0.5, 0.0, 0.0, 0.0]]]      # + infeasible, + unconstrained
    R = np.r_[S[:, 4:], [[0.5, 0, 0, 0.0], [0.5, 0, 0, 0.0]]]
    ref = Oracle(mpc._problem_dict()).solve(X, R)
    assert list(ref["status"][-2:]) == [2, 0] and np.all(ref["status"][:600] == 0)
    return X, R, ref


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
def test_bench_problem_on_both_layouts(packed, hip_lib, bench_reference, monkeypatch):
    X, R, ref = bench_reference
    mpc, _ = _make(monkeypatch, packed, "cartpole", 10, True)
    assert hip_lib.get_factoring(mpc._handle, 0) == ((120, 384, 5) if packed else (92, 412, 5))
    assert hip_lib.kernel_name(mpc._handle) == "tmpc::solve_kernel<11,1,0,5,4,0,8>"
    gold = np.load(os.path.join(common.GOLDEN, "cartpole_N10_oracle.npz"))
    out = mpc._solve(X, R)
    assert np.array_equal(out["status"], ref["status"])
    ok = ref["status"] == 0
    err, err_gold = np.max(np.abs(out["u_nom"][ok] - ref["u_nom"][ok])), np.max(np.abs(out["u_nom"][:600] - gold["u_nom"]))
    print(f"{'packed' if packed else 'unpacked'}: max |u_nom - oracle| {err:.2e}, max |u_nom - golden| {err_gold:.2e}, "
          f"mean iterations {out['iters'][:600].mean():.3f} (oracle {ref['iters'][:600].mean():.3f})")
    assert err <= ATOL_U and err_gold <= ATOL_U
    assert np.all(np.isnan(out["u_nom"][600])) and out["iters"][601] == 0
    assert abs(out["iters"][:600].mean() - ref["iters"][:600].mean()) < 2.0 and out["iters"].max() < 40
    again = mpc._solve(X, R)
    for k in OUT_KEYS:
        assert np.array_equal(out[k], again[k], equal_nan=True), k


@pytest.mark.gpu
def test_one_lane_short_stays_unpacked(hip_lib, monkeypatch):
    """Cart-pole N = 11: 51 dense functionals + the 14 of the last factored slot = 65."""
    X, R = S[::5, :4], S[::5, 4:]
    outs = []
    for packed in (True, False):
        mpc, _ = _make(monkeypatch, packed, "cartpole", 11, True)
        assert hip_lib.get_factoring(mpc._handle, 0) == (102, 412, 5)
        assert hip_lib.kernel_name(mpc._handle) == "tmpc::solve_kernel<12,1,0,5,4,0,8>"
        outs.append(mpc._solve(X, R))
    assert np.any(outs[0]["iters"] > 0)
    for k in OUT_KEYS:
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k


def _exactly_full(device):
    """Cart-pole N = 9 with two redundant copies of the input rows (shape_cases.input_box: the copies keep their rows in the condensed QP):
    50 dense functionals + the 14 of the last factored slot = 64."""
    mpc, _ = common.make_mpc("cartpole", 9, True, create=False, device=device)
    assert mpc._Uc.A.shape == (2, 1) and mpc._Uc.b[0] == mpc._Uc.b[1]
    box = shape_cases.input_box(4)
    mpc._Uc = Polytope(box.A, box.b * mpc._Uc.b[0])
    return mpc


def test_exactly_full_layout():
    mpc = _exactly_full(-1)
    h = _native.create(mpc._problem_dict(), -1)
    try:
        assert _native.get_dims(h, 0)[:2] == (10, 512) and _native.get_factoring(h, 0) == (128, 384, 5)
    finally:
        _native.destroy(h)


@pytest.mark.gpu
def test_exactly_full_dense_slot(hip_lib, oracle_lib):
    """free == need: the dense slot is full to its last lane and the MFMA pass runs all 16 k-steps."""
    mpc = _exactly_full(0)
    mpc.generate_optimization_problem(True)
    assert hip_lib.get_factoring(mpc._handle, 0) == (128, 384, 5)
    assert hip_lib.kernel_name(mpc._handle) == "tmpc::solve_kernel<11,1,0,5,4,0,8>"
    X = np.r_[S[::4, :4], [[0.0, 0.0, 0.2, 0.0], [0.5, 0.0, 0.0, 0.0]]]
    R = np.r_[S[::4, 4:], [[0.5, 0, 0, 0.0], [0.5, 0, 0, 0.0]]]
    ref = Oracle(mpc._problem_dict()).solve(X, R)
    out = mpc._solve(X, R)
    assert np.array_equal(out["status"], ref["status"]), (out["status"], ref["status"])
    ok = ref["status"] == 0
    assert ok.sum() >= 100 and np.any(ref["iters"][ok] > 5)
    err = np.max(np.abs(out["u_nom"][ok] - ref["u_nom"][ok]))
    print(f"exactly full: {ok.sum()} optimal of {len(X)}, max |u_nom - oracle| {err:.2e}")
    assert err <= ATOL_U
    assert np.all(np.isnan(out["u_nom"][ref["status"] == 2]))


@pytest.mark.gpu
def test_extended_controller_packet_received_problem_is_untouched(hip_lib, monkeypatch):
    """N = 10, extended: the packet-received problem (427 factored functionals, 43 in the last slot, 13 idle dense lanes) cannot pack and must not notice."""
    idx = np.arange(0, 600, 4)
    X, R = S[idx, :4], S[idx, 4:]
    var = np.ones(len(idx), dtype=np.uint8)
    outs = []
    for packed in (True, False):
        mpc, _ = _make(monkeypatch, packed, "cartpole", 10, True, extended=True)
        assert hip_lib.get_factoring(mpc._handle, 1) == (102, 854, 4)
        assert hip_lib.get_factoring(mpc._handle, 0) == ((120, 384, 5) if packed else (92, 412, 5))
        outs.append(mpc._solve(X, R, var))
    assert np.any(outs[0]["iters"] > 0)
    for k in OUT_KEYS:
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k


@pytest.mark.gpu
def test_closed_loop_on_a_packed_handle(hip_lib, monkeypatch):
    """64 trajectories x 12 steps at p_loss 0.3, warm-started, the reference steps at t = 6: the fused launch equals the launch pair per
    step bit for bit (the working-set records hold side ids of the handle's own layout), no tube violation, no non-optimal solve."""
    nb, T = 64, 12
    mpc, w = _make(monkeypatch, True, "cartpole", 10, True)
    assert hip_lib.get_factoring(mpc._handle, 0) == (120, 384, 5)
    p_loss = np.full(nb, 0.3)
    th, ga, dist = montecarlo.draw_realisations(nb, T, w["w_bound"], seed=17)
    ref = np.where(np.arange(T) < 6, 0.5, -0.3)
    off = mpc.run_closed_loop(p_loss, ref, th, ga, dist, warm_start=True, capture=5, fused="off")
    on = mpc.run_closed_loop(p_loss, ref, th, ga, dist, warm_start=True, capture=5, fused="on")
    assert on["fused"] and not off["fused"]
    for k in ("err2", "tube_violations", "not_optimal", "x_final", "consistent", "iters_sum", "x_traj", "x_nom_traj", "u_traj"):
        assert np.array_equal(np.asarray(on[k]), np.asarray(off[k]), equal_nan=True), k
    assert np.all(on["not_optimal"] == 0) and np.all(on["tube_violations"] == 0)


@pytest.mark.gpu
def test_N20_base_problem_keeps_its_layout(hip_lib, oracle_lib):
    """tests/golden/cartpole_N20_extended_hard_states.npy on the base problem (variant 0), solve_kernel<22,2,0,5,4,0,4>.  The layout is
    UNTOUCHED, ncc = 412: the skip of a factored slot is compiled into the bench shape alone -- with it, this one-wave-per-SIMD shape spills
    40 registers instead of 4 (tests/test_code_objects.py allows 16) -- and a shape that cannot skip is not packed."""
    D = np.load(os.path.join(common.GOLDEN, "cartpole_N20_extended_hard_states.npy"))
    X, R = np.ascontiguousarray(D[:, :4]), np.ascontiguousarray(D[:, 4:8])
    mpc, _ = common.make_mpc("cartpole", 20, True, create=True)
    assert hip_lib.kernel_name(mpc._handle) == "tmpc::solve_kernel<22,2,0,5,4,0,4>"
    nd, ncc, kc = hip_lib.get_factoring(mpc._handle, 0)
    assert nd + ncc == hip_lib.get_dims(mpc._handle, 0)[1] and (ncc, kc) == (412, 5)
    ref = Oracle(mpc._problem_dict()).solve(X, R)
    out = mpc._solve(X, R, want_traj=False)
    assert np.array_equal(out["status"], ref["status"]), (out["status"], ref["status"])
    ok = ref["status"] == 0
    assert np.all(np.isnan(out["u_nom"][ref["status"] == 2]))
    if ok.any():
        err = np.max(np.abs(out["u_nom"][ok, 0] - ref["u_nom"][ok, 0]))
        print(f"hard N = 20 states, base problem: {ok.sum()} optimal, max |u*_0 - oracle| {err:.2e}")
        assert err <= ATOL_U
