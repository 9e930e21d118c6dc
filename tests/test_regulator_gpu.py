"""The regulator QPs and their closed loop on the MI355X: the unconstrained regulator against the finite-horizon Riccati
recursion, KKT certificates of the constrained solves on the sparse QP, wave = block, infeasible states, the device loop
against a host loop of per-step solves, and the tube guarantee of Mayne et al. over a Monte Carlo."""
import numpy as np
import pytest

import regulator_problems as rp
from LinearMPCOverNetworks.montecarlo import draw_realisations_philox

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mayne(hip_lib):
    m = rp.mayne_tube(device=0)
    yield m
    m._close()


def _riccati_inputs(A, B, Q, R, N, x0):
    """u_0 .. u_{N-1} of min sum_{i<N} x'Qx + u'Ru (P_N = 0) from x0 (B, nx): the backward recursion, then forward."""
    P, Ks = np.zeros_like(Q), []
    for _ in range(N):
        K = np.linalg.solve(R + B.T @ P @ B, B.T @ P @ A)
        P = Q + A.T @ P @ (A - B @ K)
        Ks.append(K)
    Ks = Ks[::-1]
    x, u = x0.copy(), []
    for K in Ks:
        ui = -x @ K.T
        u.append(ui)
        x = x @ A.T + ui @ B.T
    return np.stack(u, axis=1)           # (B, N, nu)


def test_unconstrained_regulator_is_the_riccati_solution(hip_lib):
    m = rp.plain_double_integrator(X=False, U=False)
    try:
        x0 = np.random.default_rng(11).uniform(-5, 5, (1024, 2))
        out = m._solve_regulator(x0)
        assert np.all(out["status"] == 0)
        u_ref = _riccati_inputs(m._A, m._B, m._Q, m._R, m._N, x0)
        assert np.all(np.abs(out["u_nom"] - u_ref) <= 1e-9 * (1 + np.abs(u_ref)))
        assert np.array_equal(out["x_nom0"], x0)
    finally:
        m._close()


def _states(kind, n, rng):
    if kind == "mayne_tube":
        return np.c_[rng.uniform(-9.0, 5.0, n), rng.uniform(-3.5, 2.5, n)]
    return np.c_[rng.uniform(-9.0, 9.0, n), rng.uniform(-4.0, 4.0, n)]


@pytest.mark.parametrize("kind", ["plain_U", "plain_XU", "mayne_tube"])
def test_constrained_solves_carry_a_kkt_certificate(kind, hip_lib, mayne):
    m = mayne if kind == "mayne_tube" else rp.plain_double_integrator(X=kind == "plain_XU", U=True)
    try:
        sp = rp.SparseQP(m)
        xk = _states(kind, 4096, np.random.default_rng(5))
        out = m._solve_regulator(xk)
        st = out["status"]
        z = out["u_nom"].reshape(len(xk), -1)
        if sp.tube:
            z = np.c_[z, out["x_nom0"]]
        J = rp.row_jacobian(sp)
        patterns = set()
        for b in range(len(xk)):
            feas = rp.feasible(sp, J, xk[b])
            if not feas:
                assert st[b] == 2 and np.all(np.isnan(out["u_nom"][b])), (b, xk[b], st[b])
                continue
            assert st[b] == 0, (b, xk[b], st[b])
            viol, stat = rp.kkt(sp, J, z[b], xk[b])
            assert viol <= 1e-9, (b, viol)
            assert stat <= 1e-8, (b, stat)
            patterns.add(tuple(np.flatnonzero(sp.rows(z[b], xk[b]) > -1e-7)))
        assert len(patterns) >= 10, len(patterns)       # the batch mixes many active sets (and, plain, none at all)
        # the workgroup-per-QP kernel gives the same answers
        path = m.get_kernel_path()
        m.set_kernel_path("block" if path == "wave" else "wave")
        try:
            other = m._solve_regulator(xk)
        finally:
            m.set_kernel_path("auto")
        assert np.array_equal(other["status"], st)
        ok = st == 0
        assert np.max(np.abs(other["u_nom"][ok] - out["u_nom"][ok])) <= 1e-9
        assert np.max(np.abs(other["x_nom0"][ok] - out["x_nom0"][ok])) <= 1e-9
    finally:
        if m is not mayne:
            m._close()


def test_unconstrained_regulator_on_the_block_kernel(hip_lib):
    """No inequality rows at all: the block kernel runs on its padding rows only."""
    m = rp.plain_double_integrator(X=False, U=False)
    try:
        x0 = np.random.default_rng(12).uniform(-5, 5, (256, 2))
        a = m._solve_regulator(x0)
        m.set_kernel_path("block")
        b = m._solve_regulator(x0)
        assert np.all(a["status"] == 0) and np.all(b["status"] == 0)
        assert np.max(np.abs(a["u_nom"] - b["u_nom"])) <= 1e-9 * (1 + np.max(np.abs(a["u_nom"])))
    finally:
        m._close()


def test_infeasible_states(hip_lib, mayne):
    m = rp.plain_double_integrator(X=True, U=True)
    try:
        out = m._solve_regulator(np.array([[0.0, 5.0], [0.0, 1.0]]))        # x_2 = 5 lies outside X
        assert out["status"][0] == 2 and np.all(np.isnan(out["u_nom"][0])) and np.all(np.isnan(out["x_nom"][0]))
        assert out["status"][1] == 0
        assert m.solve_optimization_problem(np.array([0.0, 5.0])) == (None, None)
        x_mpc, u_mpc = m.solve_optimization_problem(np.array([[0.0, 5.0], [0.0, 1.0]]))
        assert np.all(np.isnan(u_mpc[0])) and np.all(np.isfinite(u_mpc[1]))
    finally:
        m._close()
    out = mayne._solve_regulator(np.array([[50.0, 50.0]]))
    assert out["status"][0] == 2 and np.all(np.isnan(out["u_nom"]))
    assert mayne.solve_optimization_problem(np.array([50.0, 50.0])) == (None, None)
    x_mpc, u_mpc = mayne.solve_optimization_problem(np.array([-5.0, -2.0]))
    assert x_mpc.shape == (2, 10) and u_mpc.shape == (1, 9)


def _mayne_starts(mayne, n, seed):
    rng = np.random.default_rng(seed)
    cand = np.c_[rng.uniform(-8.0, 4.0, 4 * n), rng.uniform(-3.0, 2.0, 4 * n)]
    st = mayne._solve_regulator(cand)["status"]
    x0 = cand[st == 0][:n]
    assert len(x0) == n
    return x0


def test_device_loop_equals_host_loop_tube(hip_lib, mayne):
    B, T = 512, 30
    x0 = _mayne_starts(mayne, B, 21)
    x0[-8:] = [[-5.0, -2.0]] * 4 + [[9.5, 1.9]] * 4      # (the last ones start close to the edge of X)
    w = np.random.default_rng(22).uniform(-0.1, 0.1, (B, T, 2))
    sets = {"X": mayne._X, "U": mayne._U, "Z": mayne._Z}
    dev = mayne.run_closed_loop(x0, T, w=w, capture=0)
    host = rp.host_loop(mayne, x0, w, sets, mayne.get_controller_gain())
    rp.compare_loops(dev, host)
    # the device generator against its host twin
    _, _, wp = draw_realisations_philox(B, T, [0.1, 0.1], seed=77, first=1000)
    dev = mayne.run_closed_loop(x0, T, seed=77, first_trajectory=1000, capture=0)
    host = rp.host_loop(mayne, x0, wp, sets, mayne.get_controller_gain())
    rp.compare_loops(dev, host)


def test_device_loop_equals_host_loop_plain(hip_lib):
    m = rp.plain_double_integrator(X=True, U=True)
    try:
        B, T = 512, 30
        rng = np.random.default_rng(31)
        x0 = np.c_[rng.uniform(-9.0, 9.0, B), rng.uniform(-2.5, 2.5, B)]      # some start outside X: they fail at step 0
        w = rng.uniform(-0.05, 0.05, (B, T, 2))
        dev = m.run_closed_loop(x0, T, w=w, capture=0)
        host = rp.host_loop(m, x0, w, {"X": m._X, "U": m._U}, None)
        assert np.any(host["fail_step"] >= 0) and np.any(host["fail_step"] < 0)
        rp.compare_loops(dev, host)
    finally:
        m._close()


def test_mayne_tube_guarantee(hip_lib, mayne):
    """Mayne, Seron, Rakovic 2005, Proposition / Theorem 1: with w in W the state stays in x_nom + Z, in X, and the input in U."""
    B, T = 4096, 30
    x0 = _mayne_starts(mayne, B, 41)
    out = mayne.run_closed_loop(x0, T, seed=2005)
    assert np.all(out["fail_step"] == -1)
    assert int(out["tube_viol"].sum()) == 0 and int(out["x_viol"].sum()) == 0 and int(out["u_viol"].sum()) == 0
    assert np.all(out["not_optimal"] == 0)
    assert np.all(np.abs(out["x_final"]) < 1.0)       # regulated into a neighbourhood of the origin
