"""Independent judges of the solution's sensitivity (test infrastructure, NOT product code).

1. `sparse_jacobian`: differentiates the UN-CONDENSED tube-tracking QP of oracle/qp_sparse.SparseTemplate (the reference's own
   variables, equalities kept) through its dense KKT matrix, working set from `minimiser_distance`, all linear algebra in
   np.longdouble.  It shares neither the condensing nor the output map with the product.
2. `planted_case` / `planted_judge`: QPs whose minimiser and working set are known by construction, and their Jacobian from the
   dense KKT matrix of the condensed form in np.longdouble.
"""
from __future__ import annotations

import numpy as np

from oracle import qp_sparse

LD = np.longdouble


def ld_solve(A, B):
    """Gaussian elimination with partial pivoting in np.longdouble (numpy.linalg has no extended precision)."""
    A = np.array(A, dtype=LD)
    X = np.array(B, dtype=LD).reshape(A.shape[0], -1)
    n = A.shape[0]
    M = np.concatenate([A, X], axis=1)
    for k in range(n):
        piv = k + int(np.argmax(np.abs(M[k:, k])))
        if M[piv, k] == 0:
            raise np.linalg.LinAlgError("singular matrix")
        if piv != k:
            M[[k, piv]] = M[[piv, k]]
        M[k] = M[k] / M[k, k]
        col = M[:, k].copy()
        col[k] = 0
        M -= np.outer(col, M[k])
    return M[:, n:]


def kkt_jacobian(H, F, GA, EA, Y, Yp):
    """J = Yp + Y dz/dp from  [H GA'; GA 0] [dz; dlam] = [-F; EA]  in longdouble."""
    nv, k = H.shape[0], GA.shape[0]
    K = np.zeros((nv + k, nv + k), dtype=LD)
    K[:nv, :nv] = H
    K[:nv, nv:] = GA.T
    K[nv:, :nv] = GA
    rhs = np.concatenate([-np.asarray(F, dtype=LD), np.asarray(EA, dtype=LD).reshape(k, np.shape(F)[1])], axis=0)
    dz = ld_solve(K, rhs)[:nv]
    return np.asarray(Yp, dtype=LD) + np.asarray(Y, dtype=LD) @ dz


# ---------------------------------------------------------------- the un-condensed QP
def output_selector(L):
    """Rows of v that make y = [u_0 .. u_{N-1} | x_0 | x_bar | u_bar] in the layout of oracle/qp_sparse."""
    return np.r_[np.arange(L.ou, L.oxb), np.arange(L.ox, L.ox + L.nx), np.arange(L.oxb, L.oxb + L.nx), np.arange(L.oub, L.oub + L.nu)]


def sparse_jacobian(tpl: qp_sparse.SparseTemplate, model, x_k, ref, sol: dict, window=(1e-7, 1e-5), weak=1e-9, want_jacobian: bool = True) -> dict:
    """d [u_nom | x_nom0 | xu_ss] / d [x_k | ref] of the un-condensed QP at the candidate solution `sol` (u_nom, x_nom0, xu_ss of one
    instance; the state trajectory is rolled out with model = (A, B)).  -> dict(judged, J (longdouble) or None, why, near: an inactive row has a
    normalised slack inside `window`; certified, active (the working set without the rows the equalities fix), distance = max |v_W - v|,
    min_slack over the inactive rows, min_mu over the working rows)."""
    qp = tpl.instance(x_k, ref)
    L = qp["layout"]
    nx, nu, N = L.nx, L.nu, L.N
    # the candidate in the reference's variables: the state trajectory follows from x_0 and u by the dynamics
    v = np.zeros(L.nvar)
    v[L.ou:L.oxb] = np.asarray(sol["u_nom"]).reshape(-1)
    v[L.xbar] = sol["xu_ss"][:nx]
    v[L.ubar] = sol["xu_ss"][nx:]
    Am, Bm = model
    xs = [np.asarray(sol["x_nom0"], dtype=np.float64).reshape(nx)]
    for u in np.asarray(sol["u_nom"], dtype=np.float64).reshape(N, nu):
        xs.append(Am @ xs[-1] + Bm @ u)
    v[L.ox:L.ou] = np.concatenate(xs)
    d = qp_sparse.minimiser_distance(qp, v)
    if not d["certified"]:
        return dict(judged=False, J=None, why="no working set certified", near=False, certified=False, active=np.zeros(0, int), distance=np.inf,
                    min_slack=0.0, min_mu=0.0)
    act = np.asarray(d["active"], dtype=int)
    vw = v + d["dv"]
    rn = np.maximum(1.0, np.linalg.norm(qp["G"], axis=1))
    slack = (qp["h"] - qp["G"] @ vw) / rn
    inactive = np.setdiff1d(np.arange(len(slack)), act)
    near = bool(np.any((slack[inactive] > window[0]) & (slack[inactive] < window[1])))
    # rows that the equalities fix altogether (a state constraint on x_0 = x_k: a function of x_k alone, not of the decision) hold no
    # direction of v: they leave the working set, as the condensed form leaves them out of its rows
    _, sa, Vta = np.linalg.svd(qp["A"], full_matrices=True)
    NA = Vta[int((sa > 1e-12 * sa[0]).sum()):].T
    free = np.linalg.norm(qp["G"][act] @ NA, axis=1) > 1e-10 * np.maximum(np.linalg.norm(qp["G"][act], axis=1), 1e-300)
    act = act[free]
    mu = np.asarray(d["mu_in"])[free] if len(d["mu_in"]) == len(free) else np.zeros(0)
    info = dict(certified=True, active=np.sort(act), distance=float(np.max(np.abs(d["dv"]))), min_slack=float(slack[inactive].min(initial=np.inf)),
                min_mu=float(mu.min(initial=np.inf)))
    if not want_jacobian:
        return dict(judged=False, J=None, why="not asked", near=near, **info)
    C = np.vstack([qp["A"], qp["G"][act]])
    rs = np.maximum(np.linalg.norm(C, axis=1), 1e-300)
    sv = np.linalg.svd(C / rs[:, None], compute_uv=False)
    if (sv > 1e-10 * sv[0]).sum() < C.shape[0]:
        return dict(judged=False, J=None, why="rank-deficient working set", near=near, **info)
    if len(mu) and mu.min() <= weak * max(1.0, np.abs(mu).max()):
        return dict(judged=False, J=None, why="weak multiplier", near=near, **info)
    if near:
        return dict(judged=False, J=None, why="inactive slack inside the window", near=True, **info)
    n, me, ma = L.nvar, qp["A"].shape[0], len(act)
    K = np.zeros((n + me + ma, n + me + ma), dtype=LD)
    K[:n, :n] = qp["P"]
    K[:n, n:n + me] = qp["A"].T
    K[n:n + me, :n] = qp["A"]
    K[:n, n + me:] = qp["G"][act].T
    K[n + me:, :n] = qp["G"][act]
    rhs = np.zeros((n + me + ma, 2 * nx), dtype=LD)
    rhs[:n, nx:] = -tpl.Qr
    rhs[n:n + me, :nx] = tpl.Bx
    rhs[n + me:, :nx] = tpl.Hx[act]
    dv = ld_solve(K, rhs)[:n]
    return dict(judged=True, J=dv[output_selector(L)], why="", near=False, **info)


# ---------------------------------------------------------------- planted QPs
def planted_case(seed: int, nv: int, nA: int, nc: int, npar: int, B: int, ny: int = 5, weak_row: bool = False, duplicate: bool = False) -> dict:
    """A QP  min 1/2 z'Hz + (F p)'z  s.t.  G z <= g0 + Ebar p  with SPD H, random G, a chosen working set A (the first row, the last
    row and rows on both sides of the 64-row boundaries first), multipliers lambda_A > 0 and the minimiser z* they imply at p_0;
    g0 is backed out so that the rows of A are tight and every other row has a slack in [0.5, 1.5].  The other B - 1 instances move p
    by a step small enough to stay on the region (checked), their minimisers from the dense KKT system.
    weak_row: the last multiplier is exactly 0 (B must be 1).  duplicate: one more row, a copy of the first row of A, directly behind it."""
    rng = np.random.default_rng(seed)
    assert nA <= min(nv, nc)
    Q, _ = np.linalg.qr(rng.standard_normal((nv, nv)))
    H = (Q * rng.uniform(1.0, 10.0, nv)) @ Q.T
    H = 0.5 * (H + H.T)
    F = rng.standard_normal((nv, npar))
    G = rng.standard_normal((nc, nv))
    Ebar = rng.standard_normal((nc, npar))
    Y = rng.standard_normal((ny, nv))
    Yp = rng.standard_normal((ny, npar))
    pref = [r for r in (0, nc - 1, 63, 64, 65, 127, 128, 2047, 2048) if 0 <= r < nc]
    pref = list(dict.fromkeys(pref))[:nA]
    rest = np.setdiff1d(np.arange(nc), pref)
    A = np.sort(np.r_[np.asarray(pref, dtype=int), rng.choice(rest, nA - len(pref), replace=False)]).astype(int)
    p0 = rng.standard_normal(npar)
    lam = rng.uniform(0.5, 1.5, nA)
    if weak_row:
        assert B == 1 and nA >= 1
        lam[-1] = 0.0
    z0 = -np.linalg.solve(H, F @ p0 + G[A].T @ lam)
    g0 = G @ z0 - Ebar @ p0 + rng.uniform(0.5, 1.5, nc)
    g0[A] = G[A] @ z0 - Ebar[A] @ p0
    # the other instances: on the same region
    K = np.block([[H, G[A].T], [G[A], np.zeros((nA, nA))]])
    P = np.tile(p0, (B, 1))
    Z = np.tile(z0, (B, 1))
    for b in range(1, B):
        step = 1e-2 * rng.uniform(-1, 1, npar)
        for _ in range(40):               # (a square, ill-conditioned G_A moves lambda a long way: the step is halved until it stays)
            P[b] = p0 + step
            sol = np.linalg.solve(K, np.r_[-F @ P[b], g0[A] + Ebar[A] @ P[b]])
            Z[b] = sol[:nv]
            slack = g0 + Ebar @ P[b] - G @ Z[b]
            if (nA == 0 or sol[nv:].min() > 0.1) and np.delete(slack, A).min(initial=1.0) > 0.1:
                break
            step = 0.5 * step
        else:
            raise AssertionError("the planted step left its region")
    case = dict(H=H, F=F, G=G, g0=g0, Ebar=Ebar, Y=Y, Yp=Yp, P=P, Z=Z, A=A, nv=nv, nc=nc, np=npar, ny=ny, B=B)
    if duplicate:
        assert nA >= 1
        a = int(A[0])
        ins = a + 1
        for key in ("G", "Ebar"):
            case[key] = np.insert(case[key], ins, case[key][a], axis=0)
        case["g0"] = np.insert(g0, ins, g0[a])
        case["A"] = np.where(A > a, A + 1, A)           # the duplicate (row a + 1) is NOT in the expected working set
        case["nc"] = nc + 1
    return case


def planted_judge(case: dict):
    """The Jacobian of a planted case in longdouble (the same for every instance: one region)."""
    A = case["A"]
    return kkt_jacobian(case["H"], case["F"], case["G"][A], case["Ebar"][A], case["Y"], case["Yp"])


def active_words(rows, nc: int):
    w = np.zeros((nc + 31) // 32, np.uint32)
    for i in rows:
        w[int(i) >> 5] |= np.uint32(1 << (int(i) & 31))
    return w


def planted_grid():
    """The shapes of the planted cases: every nv with every |A| in {0, 1, nv // 2, nv - 1, nv}; nc, np and B cycle through their lists
    (nc raised to the next listed value that holds the working set)."""
    NV = (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 127, 128)
    NC = (1, 63, 64, 65, 2049)
    NP = (1, 8, 32)
    NB = (1, 63, 65)
    out, i = [], 0
    for nv in NV:
        for nA in sorted({0, 1, nv // 2, nv - 1, nv}):
            nc = NC[i % len(NC)]
            while nc < max(nA, 1):
                nc = NC[NC.index(nc) + 1]
            out.append(dict(seed=1000 + i, nv=nv, nA=nA, nc=nc, npar=NP[i % len(NP)], B=NB[(i // 2) % len(NB)]))
            i += 1
    return out
