"""Independent judge of the gradients with respect to the QP's data and the weights (test infrastructure, NOT product code).

`judge`: per instance the KKT system  [H G_A'; G_A 0] [a; q] = [Y' ybar; 0]  of a GIVEN working set in np.longdouble (ld_solve of
tests/sensitivity_reference.py), and from it  Hbar = -1/2 sum (a z' + z a'),  Fbar = -sum a p',  pbar = Yp' ybar - F' a + Ebar_A' q.
It shares neither the factorisation nor the order of the sums with the product.

`bound`: what separates the twin (and the kernel) from the judge, entry by entry:
    amp S + 2 B 2^-52 S,   amp = 8 (nv + |A|) EPS cond(H) cond(M),   S = sum_b s_b 1 |[z_b | p_b]|'
amp is the amplification tests/test_sensitivity.py::_planted_bound uses for the solve behind a_b (forming W = G H^-1 costs cond(H), the
products with the explicit M^-1 cost cond(M), nv + |A| terms a sum); 2 B 2^-52 S is the summation over the batch in any order (the
form of e_sum in DESIGN.md 7k).  s_b is the magnitude the rounding of a_b is relative to.  a_b = H^-1 v - W_A' q is a DIFFERENCE: its
error is relative to its two terms, not to itself -- with |A| = nv the exact a_b is zero (G_A a = 0, G_A square) and what the twin
and the kernel return is the rounding of the two terms.  And a relative error of a solve is normwise, not entrywise.  So
    s_b = |H^-1 v_b|_inf + |W_A' q_b|_inf      in every row,
both from the judge's own long-double solution (W_A' q = H^-1 v - a).  (The entrywise S = sum_b |a_b| |[z_b | p_b]|' first tried is
exceeded by the |A| = nv cases of the planted grid by up to 1e16: it is zero there.)
"""
from __future__ import annotations

import numpy as np

from sensitivity_reference import LD, ld_solve

EPS = np.finfo(np.float64).eps


def judge(H, F, G, Ebar, Y, Yp, P, Z, ybar, active, live=None) -> dict:
    """`active`: one working set for the whole batch (a planted case) or a list of them, one per instance.  live: the instances that
    count (the others add nothing and get adj = 0, pbar = NaN).  -> dict(adj, pbar, Hbar, Fbar, S) in longdouble."""
    H, F, G, Ebar, Y, Yp = (np.asarray(a, dtype=LD) for a in (H, F, G, Ebar, Y, Yp))
    nv, npar = F.shape
    P = np.asarray(P, dtype=LD).reshape(-1, npar)
    Z = np.asarray(Z, dtype=LD).reshape(-1, nv)
    B = P.shape[0]
    ybar = np.asarray(ybar, dtype=LD).reshape(B, -1)
    live = np.ones(B, bool) if live is None else np.asarray(live, dtype=bool)
    shared = not isinstance(active, list)
    sets = [np.asarray(active, dtype=int)] * B if shared else [np.asarray(a, dtype=int) for a in active]
    adj = np.zeros((B, nv), dtype=LD)
    pbar = np.full((B, npar), np.nan, dtype=LD)
    smag = np.zeros(B, dtype=LD)
    groups = {}
    for b in np.flatnonzero(live):
        groups.setdefault(sets[b].tobytes(), []).append(b)
    for idx in groups.values():
        A = sets[idx[0]]
        k = len(A)
        K = np.zeros((nv + k, nv + k), dtype=LD)
        K[:nv, :nv] = H
        K[:nv, nv:] = G[A].T
        K[nv:, :nv] = G[A]
        rhs = np.zeros((nv + k, len(idx)), dtype=LD)
        rhs[:nv] = Y.T @ ybar[idx].T
        sol = ld_solve(K, rhs)
        a, q = sol[:nv].T, sol[nv:].T
        adj[idx] = a
        hv = ld_solve(H, rhs[:nv]).T
        smag[idx] = np.abs(hv).max(axis=1) + np.abs(hv - a).max(axis=1)
        pbar[idx] = ybar[idx] @ Yp - a @ F + q @ Ebar[A]
    ZP = np.concatenate([Z, P], axis=1)
    ZP[~live] = 0
    C = adj.T @ ZP
    S = np.ones((nv, 1), dtype=LD) * (smag[None, :] @ np.abs(ZP))
    return dict(adj=adj, pbar=pbar, Hbar=-0.5 * (C[:, :nv] + C[:, :nv].T), Fbar=-C[:, nv:], S=S, smag=smag)


def amplification(H, G, A) -> float:
    A = np.asarray(A, dtype=int)
    M = G[A] @ np.linalg.solve(H, G[A].T) if len(A) else np.eye(1)
    return float(8 * (H.shape[0] + len(A)) * EPS * np.linalg.cond(H) * np.linalg.cond(M))


def bound(amp: float, S, B: int, nv: int):
    """-> (bound on |Hbar - judge|, bound on |Fbar - judge|), entry by entry."""
    S = np.asarray(S, dtype=np.float64)
    e = (amp + 2.0 * B * 2.0 ** -52) * S
    return 0.5 * (e[:, :nv] + e[:, :nv].T), e[:, nv:]


def weight_map_ld(A, B, N: int, Y, Yp, Hbar, Fbar) -> dict:
    """The adjoint of the cost assembly in np.longdouble, from the model and the output map alone (Y, Yp of tmpc_sens_get_model: the rows
    of y = [u_0 .. u_{N-1} | x_0 | x_bar | u_bar] ARE the signals u_i, x_0, x_bar, u_bar as affine functions of (z, x_k); the states
    follow by the dynamics).  Error signals x_i - x_bar (Q), u_i - u_bar (R), x_N - x_bar (P), x_bar - ref (T), priced as
    H = 2 sum L'W L, F1 = 2 sum L'W Dx, F2 = 2 sum L'W Dr, hence  Wbar = sym(2 sum (L Hbar L' + L F1bar Dx' + L F2bar Dr')).
    For the handles without an eliminated terminal equality.  It shares nothing with tmpc_sens_weight_map but the formula."""
    A, B, Y, Yp, Hbar, Fbar = (np.asarray(a, dtype=LD) for a in (A, B, Y, Yp, Hbar, Fbar))
    nx, nu = B.shape
    nv = Y.shape[1]
    sig = lambda r0, r1: (Y[r0:r1], Yp[r0:r1, :nx], Yp[r0:r1, nx:])          # (L, Dx, Dr)
    u = [sig(i * nu, (i + 1) * nu) for i in range(N)]
    x = [sig(N * nu, N * nu + nx)]
    xbar, ubar = sig(N * nu + nx, N * nu + 2 * nx), sig(N * nu + 2 * nx, N * nu + 2 * nx + nu)
    for i in range(N):
        x.append(tuple(A @ a + B @ b for a, b in zip(x[i], u[i])))
    sub = lambda p, q: tuple(a - b for a, b in zip(p, q))
    ref = (np.zeros((nx, nv), dtype=LD), np.zeros((nx, nx), dtype=LD), np.eye(nx, dtype=LD))
    F1, F2 = Fbar[:, :nx], Fbar[:, nx:]
    out = dict(Qbar=np.zeros((nx, nx), dtype=LD), Rbar=np.zeros((nu, nu), dtype=LD), Pbar=np.zeros((nx, nx), dtype=LD), Tbar=np.zeros((nx, nx), dtype=LD))
    terms = [("Qbar", sub(x[i], xbar)) for i in range(N)] + [("Rbar", sub(u[i], ubar)) for i in range(N)] + [("Pbar", sub(x[N], xbar)), ("Tbar", sub(xbar, ref))]
    for key, (L, Dx, Dr) in terms:
        out[key] += 2 * (L @ Hbar @ L.T + L @ F1 @ Dx.T + L @ F2 @ Dr.T)
    return {k: 0.5 * (v + v.T) for k, v in out.items()}
