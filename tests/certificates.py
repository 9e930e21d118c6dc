"""Solver-independent certificates of the library's answers, shared by the GPU tests (NOT product code, NOT a test module).

Tracking controllers: every OPTIMAL instance must satisfy the KKT conditions of the QP as the reference states it in its own,
un-condensed variables (oracle/qp_sparse.py builds it line by line from TubeTrackingMPC.py:104-156, :253-299), and u_0 must lie
within TOL_U0 of the exact minimiser on the certified active set; every INFEASIBLE instance must be infeasible for HiGHS
(scipy.optimize.linprog, the LP solver the reference itself calls, utils_polytope.py:19).

Regulators: the same on the sparse QP of regulator_problems.SparseQP (RegulatorMPC.py:45-76), written in z = [u_0 .. u_{N-1}]
through the model's own trajectory -- not through the library's condensing."""
from __future__ import annotations

import numpy as np

import regulator_problems as rp
from oracle import qp_sparse

TOL_STAT, TOL_FEAS = 1e-7, 1e-9
# north_star's parity band is 1e-6 on u*_0; the residual-based certificate above scales with |q| (1e6 for the cart-pole)
# and lets a 1e-6 shift of u_0 through, so every answer is also measured against the exact minimiser on its certified
# active set (qp_sparse.minimiser_distance: a linear solve, no interior-point or refinement code involved)
TOL_U0 = 1e-8


def boundary_states(rng, hx_box, n, lo=0.9):
    """States with one coordinate at lo..1.0 of the tightened box, the others anywhere inside."""
    X = rng.uniform(-1, 1, (n, len(hx_box))) * hx_box
    k = rng.integers(0, len(hx_box), n)
    X[np.arange(n), k] = rng.choice([-1.0, 1.0], n) * rng.uniform(lo, 1.0, n) * hx_box[k]
    return X


def certify_outputs(mpc, X, R, out, variant=None, literal_check=None) -> dict:
    """Certifies every answer of `out` (mpc._solve(X, R, variant)); returns dict(n_opt, n_inf, worst)."""
    p = mpc._problem_dict()
    var = np.zeros(len(X), np.uint8) if variant is None else np.broadcast_to(np.asarray(variant, np.uint8), (len(X),))
    tpl = {v: qp_sparse.SparseTemplate(p, int(v)) for v in np.unique(var)}
    st = out["status"]
    assert np.all((st == 0) | (st == 2)), np.bincount(st)
    worst = dict(r_stat=0.0, r_eq=0.0, r_ineq=0.0, du0=0.0)
    n_inf = 0
    for k in range(len(X)):
        qp = tpl[var[k]].instance(X[k], R[k])
        if st[k] == 2:
            tight = dict(qp)
            tight["h"] = qp["h"] - 1e-6 * np.maximum(1.0, np.abs(qp["h"]))       # borderline instances may go either way
            assert qp_sparse.lp_infeasible(tight), f"instance {k}: library says infeasible, HiGHS finds a strictly feasible point"
            assert np.all(np.isnan(out["u_nom"][k]))
            n_inf += 1
            continue
        v = qp_sparse.pack(qp, out["x_nom"][k], out["u_nom"][k], out["x_ss"][k], out["u_ss"][k])
        c = qp_sparse.kkt_certificate_fast(qp, v)
        lam_scale = max(1.0, float(np.abs(c["lam"]).max())) if len(c["lam"]) else 1.0
        assert c["r_eq"] < TOL_FEAS and c["r_ineq"] < TOL_FEAS and c["r_stat"] < TOL_STAT and c["min_lam"] >= -1e-9 * lam_scale, (k, c)
        for key in ("r_stat", "r_eq", "r_ineq"):
            worst[key] = max(worst[key], c[key])
        d = qp_sparse.minimiser_distance(qp, v, active=c["active"])
        assert d["certified"], (k, {a: d[a] for a in ("r_ineq", "min_mu", "r_stat", "resolution", "n_active")})
        assert d["du0"] <= TOL_U0, (k, d["du0"], c["n_active"])
        worst["du0"] = max(worst["du0"], d["du0"])
        if literal_check is not None and var[k] == 1:
            literal_check(out["x_ss"][k], out["u_ss"][k])
    return dict(n_opt=int((st == 0).sum()), n_inf=n_inf, worst=worst)


def exact_distance(mpc, x_k, ref, variant, x_nom, u_nom, x_ss, u_ss) -> dict:
    """Entry-wise distance of one answer to THE minimiser (qp_sparse.minimiser_distance on its certified active set): the
    largest error over all inputs, over the steady state (x_ss, u_ss) and over the nominal trajectory, and whether the active
    set certified.  Decides which side is wrong where the library and the oracle disagree."""
    qp = qp_sparse.SparseTemplate(mpc._problem_dict(), int(variant or 0)).instance(x_k, ref)
    v = qp_sparse.pack(qp, x_nom, u_nom, x_ss, u_ss)
    d = qp_sparse.minimiser_distance(qp, v, active=qp_sparse.kkt_certificate_fast(qp, v)["active"])
    L, dv = qp["layout"], np.abs(d["dv"])
    return dict(u=float(dv[L.ou:L.oxb].max()), ss=float(max(dv[L.xbar].max(), dv[L.ubar].max())),
                x=float(dv[L.ox:L.ou].max()), certified=d["certified"])


def proven_infeasible(mpc, x_k, ref, variant=None) -> bool:
    """HiGHS finds no point at all (not only no strictly feasible one, as in certify_outputs)."""
    return qp_sparse.lp_infeasible(qp_sparse.SparseTemplate(mpc._problem_dict(), int(variant or 0)).instance(x_k, ref))


def certify(mpc, X, R, variant=None, min_optimal=128, literal_check=None):
    """Solves the batch on the GPU and certifies every answer; returns (n_optimal, n_infeasible)."""
    out = mpc._solve(X, R, variant)
    c = certify_outputs(mpc, X, R, out, variant, literal_check)
    n_opt, n_inf = c["n_opt"], c["n_inf"]
    assert n_opt >= min_optimal, (n_opt, n_inf)
    print(f"certified {n_opt} optimal (worst {c['worst']}), {n_inf} infeasible by LP")
    return n_opt, n_inf


class _ULayout:
    """qp_sparse's layout interface for the variables z = [u_0 .. u_{N-1}]: u_0 is the first nu entries."""

    def __init__(self, nu):
        self.nu = nu

    def u(self, i):
        return slice(i * self.nu, (i + 1) * self.nu)


def regulator_qp(sp: rp.SparseQP, J, xk) -> dict:
    """The sparse QP of `sp` at x_k in qp_sparse's standard form over z: min 1/2 z'Pz + q'z  s.t.  G z <= h.  The cost is
    quadratic and the rows affine in z, so P, q, G, h are read off the cost gradient and the rows of the trajectory."""
    assert not sp.tube
    g0 = sp.cost_gradient(np.zeros(sp.nv), xk)
    P = np.stack([sp.cost_gradient(e, xk) - g0 for e in np.eye(sp.nv)], axis=1)
    return dict(P=0.5 * (P + P.T), q=g0, c0=0.0, A=np.zeros((0, sp.nv)), b=np.zeros(0), G=J, h=-sp.rows(np.zeros(sp.nv), xk),
                layout=_ULayout(sp.nu))


def certify_regulator(m, X, out) -> dict:
    """Every answer of a plain regulator (m._solve_regulator(X)): INFEASIBLE exactly where HiGHS finds no z; OPTIMAL answers
    primal feasible to 1e-9, stationary to 1e-8 with NNLS multipliers on the near-active rows, and u_0 within TOL_U0 of the
    exact minimiser on the certified active set.  Returns dict(n_opt, n_inf, worst_du0)."""
    sp = rp.SparseQP(m)
    J = rp.row_jacobian(sp)
    st = out["status"]
    z = out["u_nom"].reshape(len(X), -1)
    n_inf, worst = 0, 0.0
    for b in range(len(X)):
        if not rp.feasible(sp, J, X[b]):
            assert st[b] == 2 and np.all(np.isnan(out["u_nom"][b])), (b, X[b], st[b])
            n_inf += 1
            continue
        assert st[b] == 0, (b, X[b], st[b])
        viol, stat = rp.kkt(sp, J, z[b], X[b])
        assert viol <= 1e-9, (b, viol)
        assert stat <= 1e-8, (b, stat)
        qp = regulator_qp(sp, J, X[b])
        d = qp_sparse.minimiser_distance(qp, z[b])
        assert d["certified"], (b, {a: d[a] for a in ("r_ineq", "min_mu", "r_stat", "resolution", "n_active")})
        assert d["du0"] <= TOL_U0, (b, d["du0"], d["n_active"])
        worst = max(worst, d["du0"])
    return dict(n_opt=int((st == 0).sum()), n_inf=n_inf, worst_du0=worst)
