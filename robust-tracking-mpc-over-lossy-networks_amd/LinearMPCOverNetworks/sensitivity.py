"""Sensitivity of the MPC solution to its inputs (include/tmpc.h: tmpc_sens_jacobian, tmpc_sens_vjp, tmpc_qp_sensitivity).

`qp_sensitivity` is the numpy TWIN of the kernel csrc/tmpc_sens.hip: the same working-set rule, the same row order in the rank test,
the same row-by-row factorisation with L^-1 kept, the same flags and tolerances.  It exists to pin the kernel (tests) and to
differentiate on a host-only handle; the device entry points are `_native.sens_jacobian`, `_native.sens_vjp`,
`_native.qp_sensitivity`.

The QP:  min 1/2 z'Hz + (F p)'z  s.t.  G z <= g0 + Ebar p,   y = Y z + Yp p.   On the critical region of a minimiser z with working set A
(rows with slack <= act_tol, ascending, rank-tested in that order):  M = G_A H^-1 G_A',
    lambda_A = -M^-1 (G_A H^-1 F p + g0_A + Ebar_A p),   dlambda/dp = -M^-1 (G_A H^-1 F + Ebar_A),   dz/dp = -H^-1 (F + G_A' dlambda/dp),
    J = Y dz/dp + Yp.
"""
from __future__ import annotations

import numpy as np

# include/tmpc.h: TMPC_SENS_*; csrc/tmpc_sens.hpp: SENS_*_TOL
SKIPPED, DEPENDENT, WEAK, NOT_KKT = 1, 2, 4, 8
RANK_TOL, MULT_TOL, KKT_TOL, ACT_TOL = 1e-10, 1e-9, 1e-6, 1e-7
STATUS_INFEASIBLE = 2


def _factor(cand, G, W, nv):
    """The candidates, in the order given, through the row-by-row Cholesky factorisation of M = G_A H^-1 G_A': the kept rows, L^-1
    and whether a row was dropped."""
    Li = np.zeros((nv, nv))
    kept = []
    dropped = False
    for i in cand:
        k = len(kept)
        if k >= nv:
            dropped = True
            continue
        m = G[kept + [int(i)]] @ W[i]
        l = Li[:k, :k] @ m[:k]
        d = m[k] - l @ l
        if not d > RANK_TOL * m[k]:
            dropped = True
            continue
        r = 1.0 / np.sqrt(d)
        Li[k, :k] = -r * (l @ Li[:k, :k])
        Li[k, k] = r
        kept.append(int(i))
    k = len(kept)
    return np.asarray(kept, dtype=np.int64), Li[:k, :k], dropped


def qp_sensitivity(H, F, G, g0, Ebar, Y, Yp, P, Z, status=None, act_tol: float = 0.0, mode: str = "jacobian", ybar=None) -> dict:
    """-> dict(out (B, ny, np) Jacobians or (B, np) vector-Jacobian products, flag (B,) int32, n_active (B,) int32,
    active (B, ceil(nc / 32)) uint32, lam: list of the multipliers of the kept rows)."""
    H, F, G, g0, Ebar, Y, Yp = (np.asarray(a, dtype=np.float64) for a in (H, F, G, g0, Ebar, Y, Yp))
    nv, npar = F.shape
    nc, ny = G.shape[0], Y.shape[0]
    G = G.reshape(nc, nv)
    Ebar = Ebar.reshape(nc, npar)
    P = np.asarray(P, dtype=np.float64).reshape(-1, npar)
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, nv)
    B = P.shape[0]
    vjp = mode == "vjp"
    if vjp:
        ybar = np.asarray(ybar, dtype=np.float64).reshape(B, ny)
    tol = act_tol if act_tol > 0 else ACT_TOL
    Hs = 0.5 * (H + H.T)
    Hinv = np.linalg.inv(Hs)
    Hinv = 0.5 * (Hinv + Hinv.T)
    W = G @ Hinv
    HinvF = Hinv @ F
    out = np.full((B, npar) if vjp else (B, ny, npar), np.nan)
    flag = np.zeros(B, np.int32)
    n_active = np.zeros(B, np.int32)
    active = np.zeros((B, (nc + 31) // 32), np.uint32)
    lams = [None] * B
    adj = np.zeros((B, nv))           # (reverse mode) a_b of  [H G_A'; G_A 0] [a; q] = [Y' ybar_b; 0];  zeros where SKIPPED
    cache = {}
    for b in range(B):
        p, z = P[b], Z[b]
        if (status is not None and status[b] >= STATUS_INFEASIBLE) or not (np.isfinite(p).all() and np.isfinite(z).all()) \
                or (vjp and not np.isfinite(ybar[b]).all()):
            flag[b] = SKIPPED
            continue
        slack = g0 + Ebar @ p - G @ z
        cand = np.flatnonzero(slack <= tol)
        key = cand.tobytes()
        if key not in cache:
            cache[key] = _factor(cand, G, W, nv)
        kept, Li, dropped = cache[key]
        k = len(kept)
        fl = DEPENDENT if dropped else 0
        f = F @ p
        thr = KKT_TOL * (1.0 + np.max(np.abs(f)))
        WA, EA = W[kept], Ebar[kept]
        lam = -(Li.T @ (Li @ (WA @ f + g0[kept] + EA @ p)))
        if k:
            if lam.min() <= MULT_TOL * max(1.0, np.abs(lam).max()):
                fl |= WEAK
            if lam.min() < -thr:
                fl |= NOT_KKT
        res = np.max(np.abs(f + H @ z + G[kept].T @ lam))
        if not res <= thr:
            fl |= NOT_KKT
        if vjp:
            v = Y.T @ ybar[b]
            q = Li.T @ (Li @ (WA @ v))
            x = Hinv @ v - WA.T @ q
            out[b] = Yp.T @ ybar[b] - F.T @ x + EA.T @ q
            # (the plain formula.  The kernel's adj output takes one more step, a refinement on the constraint rows,
            # a = x - W_A' M^-1 (G_A x): the exact a has G_A a = 0.  The twin stays the less accurate of the two.)
            adj[b] = x
        else:
            D = -(Li.T @ (Li @ (WA @ F + EA)))
            dz = -HinvF - WA.T @ D
            out[b] = Yp + Y @ dz
        flag[b] = fl
        n_active[b] = k
        for i in kept:
            active[b, i >> 5] |= np.uint32(1 << (i & 31))
        lams[b] = lam
    return dict(out=out, flag=flag, n_active=n_active, active=active, lam=lams, **(dict(adj=adj) if vjp else {}))


def qp_sensitivity_data(H, F, G, g0, Ebar, Y, Yp, P, Z, ybar, status=None, act_tol: float = 0.0) -> dict:
    """The numpy twin of tmpc_qp_sensitivity_data: the reverse mode of `qp_sensitivity` (same working set, same factorisation) and, from
    its a_b, the gradients of the scalar behind ybar with respect to the QP's data, summed over the batch:
        Hbar = -1/2 sum_b (a_b z_b' + z_b a_b'),   Fbar = -sum_b a_b p_b'      (SKIPPED instances add nothing)
    -> dict(pbar (B, np), adj (B, nv), Hbar (nv, nv) symmetric, Fbar (nv, np), flag, n_active)."""
    r = qp_sensitivity(H, F, G, g0, Ebar, Y, Yp, P, Z, status=status, act_tol=act_tol, mode="vjp", ybar=ybar)
    nv, npar = np.shape(F)
    live = (r["flag"] & SKIPPED) == 0
    a = r["adj"][live]
    C = a.T @ np.asarray(Z, dtype=np.float64).reshape(-1, nv)[live]
    return dict(pbar=r["out"], adj=r["adj"], Hbar=-0.5 * (C + C.T), Fbar=-(a.T @ np.asarray(P, dtype=np.float64).reshape(-1, npar)[live]),
                flag=r["flag"], n_active=r["n_active"])


def decode_active(active, nc=None):
    """Bit words of a region signature (one instance: (nwords,), or a batch: (B, nwords)) -> the sorted row indices (a list per instance)."""
    a = np.asarray(active, dtype=np.uint32)
    single = a.ndim == 1
    a = a.reshape(-1, a.shape[-1])
    bits = np.unpackbits(a.view(np.uint8).reshape(a.shape[0], -1), axis=1, bitorder="little")
    rows = [np.flatnonzero(r if nc is None else r[:nc]) for r in bits]
    return rows[0] if single else rows


def condensed_model(mpc_or_handle, variant: int = 0) -> dict:
    """The raw condensed data `qp_sensitivity` and `_native.qp_sensitivity` take, for variant `variant` of a controller or handle (device or
    host-only): H, G, g0 from tmpc_get_condensed; F = [F1 F2], Ebar = [E 0], the output map (Y, Yp) and the map Rec back from a solve's
    outputs from tmpc_sens_get_model."""
    from . import _native
    h = getattr(mpc_or_handle, "_handle", mpc_or_handle)
    c = _native.get_condensed(h, variant)
    m = _native.sens_get_model(h, variant)
    return dict(H=c["H"], G=c["G"], g0=c["g0"], **m)


def z_from_outputs(model: dict, x, ref, u_nom, x_nom0, xu_ss):
    """z of `condensed_model` from a solve's outputs: z = Rec [u_nom | x_nom0 | xu_ss | x_k | ref]."""
    B = np.asarray(x).reshape(-1, model["Yp"].shape[1] // 2).shape[0]
    cat = np.c_[np.asarray(u_nom, dtype=np.float64).reshape(B, -1), np.asarray(x_nom0, dtype=np.float64).reshape(B, -1),
                np.asarray(xu_ss, dtype=np.float64).reshape(B, -1), np.asarray(x, dtype=np.float64).reshape(B, -1),
                np.broadcast_to(np.asarray(ref, dtype=np.float64).reshape(-1, model["Yp"].shape[1] // 2), (B, model["Yp"].shape[1] // 2))]
    return cat @ model["Rec"].T


def handle_sensitivity(mpc_or_handle, x, ref, sol: dict, variant=None, act_tol: float = 0.0, mode: str = "jacobian", ybar=None) -> dict:
    """The twin on a handle's problem, as tmpc_sens_jacobian / tmpc_sens_vjp compute it on the device: one pass of `qp_sensitivity`
    per problem variant; instances whose variant id is out of range are SKIPPED.  `sol`: u_nom, x_nom0, xu_ss and (optionally) status."""
    h = getattr(mpc_or_handle, "_handle", mpc_or_handle)
    x = np.asarray(x, dtype=np.float64).reshape(-1, h.nx)
    B = x.shape[0]
    ref = np.broadcast_to(np.asarray(ref, dtype=np.float64).reshape(-1, h.nx), (B, h.nx))
    var = np.zeros(B, np.uint8) if variant is None else np.broadcast_to(np.asarray(variant, dtype=np.uint8).reshape(-1), (B,))
    ny = h.N * h.nu + 2 * h.nx + h.nu
    nvar = h.nvariants if variant is not None else 1
    nc_max = max(_dims(h, k)[1] for k in range(h.nvariants))
    out = np.full((B, 2 * h.nx) if mode == "vjp" else (B, ny, 2 * h.nx), np.nan)
    flag = np.full(B, SKIPPED, np.int32)
    n_active = np.zeros(B, np.int32)
    active = np.zeros((B, (nc_max + 31) // 32), np.uint32)
    status = sol.get("status")
    for k in range(nvar):
        idx = np.flatnonzero(var == k)
        if not len(idx):
            continue
        m = condensed_model(h, k)
        good = np.isfinite(sol["u_nom"][idx].reshape(len(idx), -1)).all(axis=1) & np.isfinite(sol["x_nom0"][idx]).all(axis=1) \
            & np.isfinite(sol["xu_ss"][idx]).all(axis=1)
        Z = z_from_outputs(m, x[idx], ref[idx], np.nan_to_num(sol["u_nom"][idx]), np.nan_to_num(sol["x_nom0"][idx]), np.nan_to_num(sol["xu_ss"][idx]))
        Z[~good] = np.nan
        r = qp_sensitivity(m["H"], m["F"], m["G"], m["g0"], m["Ebar"], m["Y"], m["Yp"], np.c_[x[idx], ref[idx]], Z,
                           status=None if status is None else np.asarray(status)[idx], act_tol=act_tol, mode=mode,
                           ybar=None if ybar is None else np.asarray(ybar, dtype=np.float64).reshape(B, ny)[idx])
        out[idx], flag[idx], n_active[idx] = r["out"], r["flag"], r["n_active"]
        active[idx, :r["active"].shape[1]] = r["active"]
    return dict(out=out, flag=flag, n_active=n_active, active=active)


def handle_weight_gradients(mpc_or_handle, x, ref, sol: dict, ybar, variant=None, act_tol: float = 0.0) -> dict:
    """The twin of tmpc_sens_vjp_weights on a handle's problem (device or host-only): `qp_sensitivity_data` per problem variant on the
    tmpc_get_condensed / tmpc_sens_get_model data, each variant's (Hbar, Fbar) through `_native.sens_weight_map`, the contributions added.
    K, K_anc and the sets are held fixed; Q, R, P, T count as independent symmetric parameters.
    -> dict(pbar (B, 2nx), Qbar, Rbar, Pbar, Tbar, flag, n_active)."""
    from . import _native
    h = getattr(mpc_or_handle, "_handle", mpc_or_handle)
    x = np.asarray(x, dtype=np.float64).reshape(-1, h.nx)
    B = x.shape[0]
    ref = np.broadcast_to(np.asarray(ref, dtype=np.float64).reshape(-1, h.nx), (B, h.nx))
    var = np.zeros(B, np.uint8) if variant is None else np.broadcast_to(np.asarray(variant, dtype=np.uint8).reshape(-1), (B,))
    ny = h.N * h.nu + 2 * h.nx + h.nu
    ybar = np.asarray(ybar, dtype=np.float64).reshape(B, ny)
    out = dict(pbar=np.full((B, 2 * h.nx), np.nan), flag=np.full(B, SKIPPED, np.int32), n_active=np.zeros(B, np.int32),
               Qbar=np.zeros((h.nx, h.nx)), Rbar=np.zeros((h.nu, h.nu)), Pbar=np.zeros((h.nx, h.nx)), Tbar=np.zeros((h.nx, h.nx)))
    status = sol.get("status")
    for k in range(h.nvariants if variant is not None else 1):
        idx = np.flatnonzero(var == k)
        if not len(idx):
            continue
        m = condensed_model(h, k)
        good = np.isfinite(sol["u_nom"][idx].reshape(len(idx), -1)).all(axis=1) & np.isfinite(sol["x_nom0"][idx]).all(axis=1) \
            & np.isfinite(sol["xu_ss"][idx]).all(axis=1)
        Z = z_from_outputs(m, x[idx], ref[idx], np.nan_to_num(sol["u_nom"][idx]), np.nan_to_num(sol["x_nom0"][idx]), np.nan_to_num(sol["xu_ss"][idx]))
        Z[~good] = np.nan
        r = qp_sensitivity_data(m["H"], m["F"], m["G"], m["g0"], m["Ebar"], m["Y"], m["Yp"], np.c_[x[idx], ref[idx]], Z, ybar[idx],
                                status=None if status is None else np.asarray(status)[idx], act_tol=act_tol)
        out["pbar"][idx], out["flag"][idx], out["n_active"][idx] = r["pbar"], r["flag"], r["n_active"]
        w = _native.sens_weight_map(h, r["Hbar"], r["Fbar"], k)
        for key in ("Qbar", "Rbar", "Pbar", "Tbar"):
            out[key] += w[key]
    return out


def _dims(h, k):
    from . import _native
    return _native.get_dims(h, k)


def local_law(mpc, x, ref, variant=None, act_tol: float = 0.0) -> dict:
    """The local control law of the controller at (x, ref): solves on the device, then differentiates the solution there.
    -> dict(J (B, ny, 2 nx), flag, n_active, active (region signature words), and the solve's outputs)."""
    return mpc.solve_with_sensitivity(x, ref, variant=variant, act_tol=act_tol)
