"""The explicit control law: a table of critical regions (include/tmpc.h: tmpc_law_*, tmpc_qp_law_eval; csrc/tmpc_law.hip).

`region_law` and `locate` are the numpy TWIN of the host code csrc/tmpc_law.cpp and of the kernel: the same rows in the same order, the
same search order, the same thresholds.  They exist to pin the kernel (tests) and to build and query a table on a host-only handle.
`ExplicitLaw` wraps a controller's handle: learn regions from solved instances, evaluate the law, or solve with the law in front of
the solver.

The QP:  min 1/2 z'Hz + (F p)'z  s.t.  G z <= g0 + Ebar p  (and the rows 0 <= gp0 + Ep p that depend on p only),  y = Y z + Yp p.  On
the region of a working set A, with M = G_A H^-1 G_A' and W = G H^-1:
    lambda_A = Kl p + kl,  Kl = -M^-1 (W_A F + Ebar_A),  kl = -M^-1 g0_A;    z = Kz p + kz,  Kz = -H^-1 (F + G_A' Kl),  kz = -H^-1 G_A' kl;
    y = Ky p + ky,  Ky = Y Kz + Yp,  ky = Y kz.
The region's polyhedron S p + s >= 0 has nc + npar rows: row i < nc outside A is the slack g0_i + Ebar_i p - G_i z(p) + FEAS_TOL, row
i < nc inside A is lambda_i(p) + MULT_TOL, row nc + j is gp0_j + Ep_j p + FEAS_TOL.  A p that a region accepts satisfies the KKT
conditions of the strictly convex QP there: the region's y is the minimiser's.
"""
from __future__ import annotations

import numpy as np

from .sensitivity import condensed_model, decode_active

# include/tmpc.h: TMPC_LAW_FEAS_TOL, TMPC_LAW_MULT_TOL; csrc/tmpc_law.hpp
FEAS_TOL, MULT_TOL = 1e-10, 1e-10
RANK_TOL = 1e-13                          # csrc/tmpc_law.hpp: LAW_RANK_TOL
# ExplicitLaw's default for max_tries: beyond it a miss costs more than the solve it avoids (from scripts/gpu_law.py)
DEFAULT_MAX_TRIES = 360


def law_model(mpc_or_handle, variant: int = 0) -> dict:
    """`sensitivity.condensed_model` plus the parameter-only rows as `region_law` takes them: gp0 (npar,), Ep (npar, 2 nx)."""
    from . import _native
    h = getattr(mpc_or_handle, "_handle", mpc_or_handle)
    m = condensed_model(h, variant)
    pr = _native.get_param_rows(h, variant)
    m["gp0"] = pr["gp0"]
    m["Ep"] = np.c_[pr["Ep"], np.zeros_like(pr["Ep"])]
    return m


def region_law(model: dict, rows):
    """The law of the working set `rows` (indices into the rows of G) -> dict(rows, Ky, ky, Kz, kz, Kl, kl, S, s), or None where the rows
    are dependent.  model: H, F, G, g0, Ebar, Y, Yp and optionally gp0, Ep.

    As csrc/tmpc_law.cpp: with H = L L' and V = L^-1 G_A', M = V'V and its Cholesky factor is the R of V = Q R -- M is never formed (its
    condition reaches 5e11 on the cart-pole's working sets).  In w = L'z:  w = -(Ft p + V lambda), V'w = Ebar_A p + g0_A, Ft = L^-1 F, so
    R lambda = -(Q'Ft p + R^-T (Ebar_A p + g0_A))."""
    H, F, G, g0, Ebar, Y, Yp = (np.asarray(model[k], dtype=np.float64) for k in ("H", "F", "G", "g0", "Ebar", "Y", "Yp"))
    nv, npar = F.shape
    nc = g0.shape[0]
    G, Ebar = G.reshape(nc, nv), Ebar.reshape(nc, npar)
    A = np.asarray(sorted(int(i) for i in rows), dtype=np.int64)
    if len(A) > nv or (len(A) and (A[0] < 0 or A[-1] >= nc)):
        return None
    L = model.get("_L")
    if L is None:
        L = model["_L"] = np.linalg.cholesky(0.5 * (H + H.T))
        model["_Ft"] = np.c_[np.linalg.solve(L, F), np.zeros(nv)]
    Ft = model["_Ft"]
    k = len(A)
    if k:
        V = np.linalg.solve(L, G[A].T)
        Q, Rr = np.linalg.qr(V)
        diag = np.abs(np.diag(Rr))
        if not np.all(diag > RANK_TOL * np.linalg.norm(V, axis=0).max()):
            return None
        c = np.c_[Ebar[A], g0[A]]
        X = -np.linalg.solve(Rr, Q.T @ Ft + np.linalg.solve(Rr.T, c))
        Kzz = np.linalg.solve(L.T, -(Ft + V @ X))
    else:
        X = np.zeros((0, npar + 1))
        Kzz = np.linalg.solve(L.T, -Ft)
    Kl, kl, Kz, kz = X[:, :npar], X[:, npar], Kzz[:, :npar], Kzz[:, npar]
    if not np.isfinite(Kzz).all():
        return None
    gp0 = np.asarray(model.get("gp0", np.zeros(0)), dtype=np.float64)
    Ep = np.asarray(model.get("Ep", np.zeros((0, npar))), dtype=np.float64).reshape(len(gp0), npar)
    S = np.r_[Ebar - G @ Kz, Ep]
    s = np.r_[g0 - G @ kz + FEAS_TOL, gp0 + FEAS_TOL]
    S[A], s[A] = Kl, kl + MULT_TOL
    return dict(rows=A, Ky=Y @ Kz + Yp, ky=Y @ kz, Kz=Kz, kz=kz, Kl=Kl, kl=kl, S=S, s=s)


_M64 = (1 << 64) - 1
HOP_STATS = ("chain_hits", "chain_tests", "ended_absent", "ended_cap", "ended_cycle", "ended_param_row")      # include/tmpc.h: tmpc_law_get_hop_stats


def key_bit(i: int) -> int:
    """include/tmpc.h: z(i), splitmix64 of i + 1."""
    x = ((int(i) + 1) * 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def signature_key(rows) -> int:
    """The key of the working set `rows` (include/tmpc.h): the XOR of z(i) over its rows; 0 for the empty set."""
    k = 0
    for i in set(int(i) for i in rows):
        k ^= key_bit(i)
    return k


NO_KEY = _M64                             # csrc/tmpc_law.hpp: LAW_NO_KEY, the key of a region without a working set


def hash_slots(keys):
    """The open-addressed table over the regions' keys as csrc/tmpc_law.cpp builds it (include/tmpc.h): n_slot the power of two
    >= max(64, 2 R), ids in increasing order at key & (n_slot - 1) with linear probing, a key already present keeps the earlier id, a
    region without a key (NO_KEY) is left out -> slot (n_slot,) int32, -1: empty."""
    n = 64
    while n < 2 * len(keys):
        n *= 2
    slot = np.full(n, -1, np.int32)
    for i, k in enumerate(keys):
        if int(k) == NO_KEY:
            continue
        j = int(k) & (n - 1)
        while slot[j] >= 0 and int(keys[slot[j]]) != int(k):
            j = (j + 1) & (n - 1)
        if slot[j] < 0:
            slot[j] = i
    return slot


def hash_find(keys, slot, key: int) -> int:
    """The lookup of the kernel (csrc/tmpc_law_wave.hpp: law_lookup): the id under `key`, -1 where the probe reaches an empty slot."""
    n = len(slot)
    j = int(key) & (n - 1)
    for _ in range(n):
        if slot[j] < 0:
            return -1
        if int(keys[slot[j]]) == int(key):
            return int(slot[j])
        j = (j + 1) & (n - 1)
    return -1


def locate(table, P, hint=None, order=None, max_tries: int = 0, max_hops: int = 0, nc=None, stats=None):
    """The kernel's search (csrc/tmpc_law_wave.hpp: law_find).  Per instance a chain, then a walk, at most max_tries candidates in all
    (<= 0: all); the first region tested with S p + s >= 0 in every row wins.  The chain starts at the hint where it is a valid id, with
    max_hops > 0 otherwise at order[0]; a region that fails hands over to the region whose working set differs in the LOWEST failing row,
    and the chain ends -- the conditions in this order -- at a row >= nc (default: every row is a constraint's), at an entry that is None,
    at a neighbour the table does not hold (of equal sets the first counts), at the region the chain came from, after max_hops hops, at
    max_tries.  With max_hops = 0 the chain is the hint alone.  The walk is `order` (default: 0 .. R-1) without the chain's start.  An
    entry of `table` that is None (a refused set) holds no p.  stats: an int64 array (6,) (HOP_STATS) that the chains add to.
    -> region (B,) int32 (-1: a miss), tries (B,) int32, y (B, ny) (NaN for a miss and for a non-finite p, whose tries are 0)."""
    P = np.asarray(P, dtype=np.float64)
    P = P.reshape(-1, P.shape[-1])
    B, R = P.shape[0], len(table)
    order = np.arange(R) if order is None else np.asarray(order, dtype=np.int64).reshape(-1)
    hint = np.full(B, -1) if hint is None else np.broadcast_to(np.asarray(hint, dtype=np.int64).reshape(-1), (B,))
    ny = next((t["Ky"].shape[0] for t in table if t is not None), 0)
    region, tries, y = np.full(B, -1, np.int32), np.zeros(B, np.int32), np.full((B, ny), np.nan)
    index = {}
    if max_hops > 0:
        for r, t in enumerate(table):
            if t is not None:
                index.setdefault(frozenset(int(i) for i in t["rows"]), r)

    def fail_row(r, p):
        """The lowest failing row of region r at p, -1: none."""
        t = table[r]
        if t is None:
            return 0
        bad = np.flatnonzero(~(t["S"] @ p + t["s"] >= 0.0))
        return int(bad[0]) if len(bad) else -1

    for b in range(B):
        p = P[b]
        if not np.isfinite(p).all():
            continue
        hinted = 0 <= hint[b] < R
        start = int(hint[b]) if hinted else (int(order[0]) if max_hops > 0 and len(order) else -1)
        if start >= 0:
            r, prev, hops, end = start, -1, 0, None
            while True:
                tries[b] += 1
                i = fail_row(r, p)
                if max_hops > 0 and stats is not None:
                    stats[1] += 1
                if i < 0:
                    region[b], end = r, 0
                    break
                if max_hops <= 0:
                    break
                t = table[r]
                if t is not None and i >= (len(t["s"]) if nc is None else nc):
                    end = 5
                    break
                if t is None:
                    break
                nb = index.get(frozenset(int(j) for j in t["rows"]) ^ {i}, -1)
                if nb < 0:
                    end = 2
                    break
                if nb == prev:
                    end = 4
                    break
                if hops == max_hops:
                    end = 3
                    break
                if max_tries > 0 and tries[b] == max_tries:
                    break
                prev, r, hops = r, nb, hops + 1
            if max_hops > 0 and stats is not None and end is not None:
                stats[end] += 1
        if region[b] < 0:
            for r in order:
                if max_tries > 0 and tries[b] >= max_tries:
                    break
                if r == start:
                    continue
                tries[b] += 1
                if fail_row(int(r), p) < 0:
                    region[b] = r
                    break
        if region[b] >= 0:
            t = table[region[b]]
            y[b] = t["Ky"] @ p + t["ky"]
    return region, tries, y


def words_of(rows, nc: int):
    """Row indices -> the bit words of a region signature (ceil(nc / 32),) uint32."""
    w = np.zeros((nc + 31) // 32, np.uint32)
    for i in rows:
        w[int(i) >> 5] |= np.uint32(1 << (int(i) & 31))
    return w


class ExplicitLaw:
    """The explicit law of a controller (TubeTrackingMPC.explicit_law()): a table of region laws per problem variant on the
    controller's handle, filled from instances the solver has answered.

        law = mpc.explicit_law()
        out = law.solve(x, ref, hint=last_region)      # hits from the table, misses from the solver; out["region"] tells which
        law.learn(x[out["region"] < 0], ref)           # every few steps: the regions of the misses

    `max_tries` bounds the candidates tested per instance (None: DEFAULT_MAX_TRIES; 0: all)."""

    def __init__(self, mpc):
        self._mpc = mpc

    @property
    def _h(self):
        h = self._mpc._handle
        if h is None:
            raise RuntimeError("setup_optimization() has not been called")
        return h

    def learn(self, x, ref, variant=None, act_tol: float = 0.0):
        """Solves the instances on the device and adds the regions of their working sets -> (ids (B,), number of new regions)."""
        from . import _native
        out = self._mpc._solve(x, ref, variant=variant, want_traj=False)
        xs = np.asarray(x, dtype=np.float64).reshape(-1, self._h.nx)
        return _native.law_learn(self._h, xs, ref, out, variant=variant, act_tol=act_tol)

    def learn_from_misses(self, result, act_tol: float = 0.0):
        """The regions of the steps a closed loop through the law missed (run_closed_loop(law=dict(miss_capacity=..)): `result` is what
        it returned, or the dict of _native.mc_law_misses): solves the logged [x_hat | ref_k] and learns them -> (ids, number of new
        regions).  A pilot sweep with an empty table and a full log, then this, is the table of the sweep that follows."""
        m = result["law_misses"]() if "law_misses" in result else result
        if len(m["x_k"]) == 0:
            return np.zeros(0, np.int32), 0
        return self.learn(m["x_k"], m["ref"], variant=m["variant"] if self._h.nvariants > 1 else None, act_tol=act_tol)

    def add(self, words, variant: int = 0):
        """Adds working sets given as bit words (sensitivity's `active`) -> ids."""
        from . import _native
        return _native.law_add(self._h, words, variant)

    def evaluate(self, x, ref, variant=None, hint=None, max_tries=None, want_traj: bool = True) -> dict:
        """The law alone: the outputs of `_solve` plus region and tries; a miss has NaN outputs, status 3 and region -1."""
        from . import _native
        return _native.law_eval(self._h, x, ref, variant, hint, DEFAULT_MAX_TRIES if max_tries is None else max_tries, want_traj)

    def solve(self, x, ref, variant=None, hint=None, max_tries=None, want_traj: bool = True) -> dict:
        """The law with the solver behind it: every instance answered as by `_solve`; region >= 0 where the table answered."""
        from . import _native
        return _native.law_solve(self._h, x, ref, variant, hint, DEFAULT_MAX_TRIES if max_tries is None else max_tries, want_traj)

    def set_hops(self, n: int):
        """tmpc_law_set_hops: a search whose hint (or first candidate) fails hops to the neighbouring region across the failing row, at
        most n times, before it walks the search order; 0: off.  Handle-wide: evaluate, solve and the closed loops through the law."""
        from . import _native
        _native.law_set_hops(self._h, n)

    @property
    def max_hops(self) -> int:
        from . import _native
        return _native.law_get_hops(self._h)

    def hop_stats(self, variant: int = 0, clear: bool = False) -> dict:
        """The chains' counters of a variant since the table was cleared (HOP_STATS); clear: zero them after reading."""
        from . import _native
        return dict(zip(HOP_STATS, (int(v) for v in _native.law_hop_stats(self._h, variant, clear))))

    def reorder(self, variant=None):
        """Sorts the search order by descending hits (ties by id); the ids stay."""
        from . import _native
        for k in range(self._h.nvariants) if variant is None else (variant,):
            _native.law_reorder(self._h, k)

    def clear(self, variant=None):
        from . import _native
        for k in range(self._h.nvariants) if variant is None else (variant,):
            _native.law_clear(self._h, k)

    def region(self, i: int, variant: int = 0) -> dict:
        """Region i as uploaded: rows (the working set), words, Ky, ky, S, s."""
        from . import _native
        r = _native.law_get_region(self._h, i, variant)
        r["rows"] = decode_active(r["words"], nc=_native.get_dims(self._h, variant)[1])
        return r

    def hits_of(self, variant: int = 0):
        from . import _native
        return _native.law_stats(self._h, variant)

    @property
    def hits(self):
        """The hit counters of variant 0 (R,) int64 (`hits_of(k)` for another variant)."""
        return self.hits_of(0)

    @property
    def n_regions(self) -> int:
        """Regions stored, over all variants."""
        return int(sum(len(self.hits_of(k)) for k in range(self._h.nvariants)))
