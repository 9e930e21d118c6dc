"""The clipped family of the explicit-law tests (NOT a test module): the QP  min 1/2 z'Dz + (F p)'z  over a box has the closed-form
minimiser z_i = clip(-(F p)_i / d_i, -1, 1) and a closed-form working set, so the table, the search and the kernel can be judged without a
solver.

Rows.  The box rows are [I; -I] (z_i <= 1 is row i, -z_i <= 1 is row nv + i).  A case with nc rows keeps the first min(nc, 2 nv) of them --
with nc < 2 nv the variables whose row is missing are unbounded on that side and the clip is one-sided -- and fills up to nc with padding
rows g'z <= 1e6 + e'p that never bind (|z_i| <= max(1, |(F p)_i / d_i|) < 1e3 by construction).
Margins.  Every p is drawn until every |(F p)_i / d_i| is at least 0.1 away from 1: slacks and multipliers of the right region are at
least 0.1 min(d) = 0.05, nine orders above the acceptance thresholds and rounding, so region and tries are decided and no case is left out."""
import numpy as np

from LinearMPCOverNetworks import explicit_law as E


def clipped_case(seed: int, nv: int, nc: int, npar: int, B: int) -> dict:
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.5, 2.0, nv)
    # rows of F at two scales, so that most ratios lie far from 1 on either side and the rejection below ends quickly
    scale = np.where(np.arange(nv) % 2 == 0, 20.0, 0.05)
    F = rng.standard_normal((nv, npar)) * (scale / np.sqrt(npar))[:, None]
    nbox = min(nc, 2 * nv)
    box = np.r_[np.eye(nv), -np.eye(nv)][:nbox]
    G, g0, Ebar = np.zeros((nc, nv)), np.ones(nc), np.zeros((nc, npar))
    G[:nbox] = box
    G[nbox:] = rng.standard_normal((nc - nbox, nv))
    Ebar[nbox:] = 0.1 * rng.standard_normal((nc - nbox, npar))
    g0[nbox:] = 1e6
    P = np.zeros((B, npar))
    for b in range(B):
        for _ in range(10000):
            p = rng.standard_normal(npar)
            r = F @ p / d
            if np.all(np.abs(np.abs(r) - 1.0) >= 0.1) and np.abs(r).max() < 1e3:
                break
        else:
            raise RuntimeError("no p with margins")
        P[b] = p
    has_up, has_lo = np.arange(nv) < nbox, nv + np.arange(nv) < nbox
    Rr = -(P @ F.T) / d
    Z = np.where(has_up & (Rr > 1.0), 1.0, np.where(has_lo & (Rr < -1.0), -1.0, Rr))
    sets = [sorted(list(np.flatnonzero(has_up & (Rr[b] > 1.0))) + list(nv + np.flatnonzero(has_lo & (Rr[b] < -1.0)))) for b in range(B)]
    model = dict(H=np.diag(d), F=F, G=G, g0=g0, Ebar=Ebar, Y=np.eye(nv), Yp=np.zeros((nv, npar)))
    return dict(model=model, nv=nv, nc=nc, npar=npar, B=B, P=P, Z=Z, sets=sets, has_up=has_up, has_lo=has_lo, rng=rng)


def other_patterns(c: dict, n: int, avoid):
    """n working sets (sign patterns over the box rows that exist) that are none of `avoid`."""
    seen, out, nv = {tuple(a) for a in avoid}, [], c["nv"]
    guard = 0
    while len(out) < n:
        guard += 1
        pat = c["rng"].integers(-1, 2, nv)
        if guard > 1000:                  # (nv = 1 with one row: fewer patterns exist than asked for -- repeat the empty set's complement)
            break
        rows = tuple(sorted([i for i in range(nv) if pat[i] > 0 and c["has_up"][i]] + [nv + i for i in range(nv) if pat[i] < 0 and c["has_lo"][i]]))
        if rows not in seen:
            seen.add(rows)
            out.append(list(rows))
    return out


def table_of(c: dict, R: int):
    """R working sets: the distinct sets of the instances in order of first appearance, cut or filled with other patterns to R (where fewer
    than R patterns exist at all, sets repeat) -> (list of row lists, words (R, ceil(nc / 32)))."""
    sets = []
    for s in c["sets"]:
        if s not in sets:
            sets.append(s)
    sets = sets[:R]
    sets += other_patterns(c, R - len(sets), sets)
    while len(sets) < R:
        sets.append(sets[len(sets) % max(1, len(sets))])
    words = np.array([E.words_of(s, c["nc"]) for s in sets], dtype=np.uint32).reshape(R, (c["nc"] + 31) // 32)
    return sets, words
