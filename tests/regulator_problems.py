"""The regulator problems of the tests (the reference's two regulator examples and the cart-pole) and their un-condensed QPs
written out in numpy: the independent statement the condensed form of tmpc_create_regulator is checked against.  NOT product
code."""
from __future__ import annotations

import numpy as np
from scipy.optimize import linprog, nnls

import common  # noqa: F401  (sys.path)
from LinearMPCOverNetworks import _native, workloads
from LinearMPCOverNetworks.polytope_lite import Polytope
from LinearMPCOverNetworks.RegulatorMPC import RegulatorMPC
from LinearMPCOverNetworks.TubeRegulatorMPC import TubeRegulatorMPC

U_UNIT = Polytope(np.array([[1.0], [-1.0]]), np.ones(2))


def plain_double_integrator(X: bool = False, U: bool = True, device: int = 0, create: bool = True) -> RegulatorMPC:
    """Example_of_Regulator_MPC.py: A = [[1,1],[0,1]], B = [0,1]', Q = I, R = 1, N = 10, U = [-1, 1]; with X: |x_i| <= (10, 2)."""
    m = RegulatorMPC(np.array([[1.0, 1.0], [0.0, 1.0]]), np.array([[0.0], [1.0]]), np.eye(2), np.eye(1), 10)
    if U:
        m.set_input_constraints(U_UNIT)
    if X:
        m.set_state_constraints(Polytope(np.r_[np.eye(2), -np.eye(2)], np.array([10.0, 2.0, 10.0, 2.0])))
    m.set_device(device)
    if create:
        m.generate_optimization_problem()
    return m


def mayne_tube(device: int = 0) -> TubeRegulatorMPC:
    """Example_of_Tube_Regulator_MPC.py (Mayne, Seron, Rakovic 2005, section 4.1): A = [[1,1],[0,1]], B = [0.5, 1]', Q = I,
    R = 0.01, N = 9, U = [-1, 1], X = {|x_1| <= 10, -10 <= x_2 <= 2}, W = 0.1-box."""
    m = TubeRegulatorMPC(np.array([[1.0, 1.0], [0.0, 1.0]]), np.array([[0.5], [1.0]]), np.eye(2), 0.01 * np.eye(1), 9)
    m.set_input_constraints(U_UNIT)
    m.set_state_constraints(Polytope(np.r_[np.eye(2), -np.eye(2)], np.array([10.0, 2.0, 10.0, 10.0])))
    m.set_device(device)
    m.setup_optimization(Polytope(np.r_[np.eye(2), -np.eye(2)], 0.1 * np.ones(4)))
    return m


def cartpole_plain(device: int = 0) -> RegulatorMPC:
    """The cart-pole model of the result scripts with its X and U, regulated to the origin (N = 10)."""
    w = workloads.cartpole()
    m = RegulatorMPC(w["A"], w["B"], w["Q"], w["R"], 10)
    m.set_input_constraints(w["U"])
    m.set_state_constraints(w["X"])
    m.set_device(device)
    m.generate_optimization_problem()
    return m


class SparseQP:
    """The QP of RegulatorMPC.py:45-76 / TubeRegulatorMPC.py:109-143 in the variables (x_0 .. x_N, u_0 .. u_{N-1}), with
    z = [u_0 .. u_{N-1} (| x_0 for the tube)] as the condensed form orders it."""

    def __init__(self, m: RegulatorMPC):
        self.m = m
        self.d = m._regulator_dict()
        self.nx, self.nu, self.N = m._nx, m._nu, m._N
        self.tube = bool(self.d["tube"])
        self.nv = self.N * self.nu + (self.nx if self.tube else 0)

    def trajectory(self, z, xk):
        nx, nu, N = self.nx, self.nu, self.N
        u = z[:N * nu].reshape(N, nu)
        x = np.empty((N + 1, nx))
        x[0] = z[N * nu:] if self.tube else xk
        for i in range(N):
            x[i + 1] = self.m._A @ x[i] + self.m._B @ u[i]
        return x, u

    def cost(self, z, xk):
        x, u = self.trajectory(z, xk)
        Q, R = self.m._Q, self.m._R
        c = sum(x[i] @ Q @ x[i] + u[i] @ R @ u[i] for i in range(self.N))
        if self.tube:
            c += x[self.N] @ self.d["P"] @ x[self.N]
        return c

    def cost_gradient(self, z, xk):
        """d cost / d z through the adjoint recursion of the dynamics."""
        x, u = self.trajectory(z, xk)
        A, B, Q, R, N, nu = self.m._A, self.m._B, self.m._Q, self.m._R, self.N, self.nu
        lam = 2 * self.d["P"] @ x[N] if self.tube else np.zeros(self.nx)      # d cost / d x_N
        g = np.zeros(self.nv)
        for i in range(N - 1, -1, -1):
            g[i * nu:(i + 1) * nu] = 2 * R @ u[i] + B.T @ lam
            lam = 2 * Q @ x[i] + A.T @ lam
        if self.tube:
            g[N * nu:] = lam
        return g

    def rows(self, z, xk):
        """H (signal) - h for every row, in the reference's order, and for each row whether it depends on z."""
        x, u = self.trajectory(z, xk)
        d, out = self.d, []
        if self.tube:
            out.append(d["HZ"] @ (xk - x[0]) - d["hZ"])
        for i in range(self.N):
            if d.get("Hx") is not None:
                out.append(d["Hx"] @ x[i] - d["hx"])
            if d.get("Hu") is not None:
                out.append(d["Hu"] @ u[i] - d["hu"])
        if d.get("Hf") is not None:
            out.append(d["Hf"] @ x[self.N] - d["hf"])
        return np.concatenate(out) if out else np.zeros(0)

    def z_dependent_rows(self):
        rng = np.random.default_rng(1)
        xk, z = rng.standard_normal(self.nx), rng.standard_normal(self.nv)
        base = self.rows(z, xk)
        J = np.stack([self.rows(z + e, xk) - base for e in np.eye(self.nv)], axis=1) if base.size else np.zeros((0, self.nv))
        return np.abs(J).max(axis=1, initial=0.0) > 1e-12 if base.size else np.zeros(0, bool)


# ------------------------------------------------------------- checks of the solves and of the closed loop (the GPU tests)
def row_jacobian(sp):
    """The rows are affine in z: rows(z, x_k) = J z + rows(0, x_k)."""
    xk = np.zeros(sp.nx)
    base = sp.rows(np.zeros(sp.nv), xk)
    return np.stack([sp.rows(e, xk) - base for e in np.eye(sp.nv)], axis=1)


def feasible(sp, J, xk):
    """Is the sparse QP feasible at x_k?  (an LP in z over its rows)"""
    base = sp.rows(np.zeros(sp.nv), xk)
    r = linprog(np.zeros(sp.nv), A_ub=J, b_ub=-base, bounds=[(None, None)] * sp.nv, method="highs")
    return r.status == 0


def kkt(sp, J, z, xk):
    """(max primal violation, stationarity residual) of z on the sparse QP, multipliers by NNLS on the near-active rows."""
    base = sp.rows(np.zeros(sp.nv), xk)
    s = sp.rows(z, xk)
    g = sp.cost_gradient(z, xk)
    act = s >= -1e-7 * (1 + np.abs(base)) if s.size else np.zeros(0, bool)
    if act.any():
        lam, _ = nnls(J[act].T, -g)
        res = g + J[act].T @ lam
    else:
        res = g
    viol = float(np.max(s, initial=-np.inf)) if s.size else 0.0
    return viol, float(np.max(np.abs(res))) / (1.0 + float(np.max(np.abs(g))))


def host_loop(m, x0, w, sets, K):
    """The loop of Example_of_Tube_Regulator_MPC.py in numpy around per-step batch solves (tmpc_solve_batch)."""
    B, T, nx = w.shape
    x = x0.copy()
    res = dict(cost=np.zeros(B), x_viol=np.zeros(B, np.int32), u_viol=np.zeros(B, np.int32), tube_viol=np.zeros(B, np.int32),
               not_optimal=np.zeros(B, np.int32), fail_step=np.full(B, -1, np.int32), iters_sum=np.zeros(B, np.int32))
    xs, xns, us = [x[0].copy()], [], []
    viol = lambda P, v: np.any(v @ P.A.T - P.b > 1e-7, axis=1)      # noqa: E731
    for t in range(T):
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
        for key, P, v in (("x_viol", sets.get("X"), x), ("u_viol", sets.get("U"), u), ("tube_viol", sets.get("Z"), x - xn)):
            if P is not None:
                res[key] += go & viol(P, v)
        xp = x @ m._A.T + u @ m._B.T + w[:, t]
        x = np.where(go[:, None], xp, x)
        xs.append(x[0].copy()); xns.append(xn[0].copy()); us.append(u[0].copy())
    res["x_final"] = x
    res["x_traj"], res["x_nom_traj"], res["u_traj"] = np.array(xs), np.array(xns), np.array(us)
    return res


def compare_loops(dev, host):
    assert np.all(np.abs(dev["x_final"] - host["x_final"]) <= 1e-12 * (1 + np.abs(host["x_final"])))
    assert np.all(np.abs(dev["cost"] - host["cost"]) <= 1e-12 * (1 + np.abs(host["cost"])))
    for k in ("x_viol", "u_viol", "tube_viol", "not_optimal", "fail_step", "iters_sum"):
        assert np.array_equal(dev[k], host[k]), k
    for k in ("x_traj", "x_nom_traj", "u_traj"):
        assert np.allclose(dev[k], host[k], rtol=1e-12, atol=1e-12, equal_nan=True), k
