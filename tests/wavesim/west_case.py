"""TEST INFRASTRUCTURE: drives tests/wavesim/westsim_* (csrc/tmpc_west.hip on the host execution model; the file formats are
described in westsim_main.cpp)."""

import numpy as np

from hostsim import run_files


def run_select(binary, data, ranks, env=None):
    """data: (n, ncol) or (n,); returns dict(order_stats (ncol, n_rank), n_nonfinite (ncol), rendezvous, stderr)"""
    d = np.asarray(data, dtype=np.float64)
    d = d.reshape(-1, 1) if d.ndim == 1 else d
    n, ncol = d.shape
    rk = np.asarray(ranks, dtype=np.int64).reshape(-1)
    raw, err = run_files(binary, "select", [np.array([n, ncol, rk.size], dtype=np.int64), rk, d.T], env)
    k = ncol * rk.size
    return dict(order_stats=np.frombuffer(raw, dtype=np.float64, count=k).reshape(ncol, rk.size).copy(),
                n_nonfinite=np.frombuffer(raw, dtype=np.int64, count=ncol, offset=8 * k).copy(),
                rendezvous=int(np.frombuffer(raw, dtype=np.int64, count=1, offset=8 * (k + ncol))[0]), stderr=err)


def run_rollout(binary, Acl, K, par7, T, substeps=10, x0=None, box=None, n_traj=None, seed=0, first=0, env=None):
    """returns dict(x0_used (n, 4), samples (4, T - 1, n), xnorm (n), min (4), max (4), stderr)"""
    draw = x0 is None
    n = int(n_traj) if draw else np.asarray(x0).reshape(-1, 4).shape[0]
    lo, hi = box if draw else (np.zeros(4), np.zeros(4))
    payload = [np.asarray(Acl, dtype=np.float64), np.asarray(K, dtype=np.float64).reshape(4), np.asarray(par7, dtype=np.float64),
               np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64),
               np.array([substeps, T, int(draw), n, first, seed], dtype=np.int64)]
    if not draw:
        payload.append(np.asarray(x0, dtype=np.float64).reshape(-1, 4))
    raw, err = run_files(binary, "rollout", payload, env)
    o = np.frombuffer(raw, dtype=np.float64)
    ns = 4 * (T - 1) * n
    return dict(x0_used=o[:4 * n].reshape(n, 4).copy(), samples=o[4 * n:4 * n + ns].reshape(4, T - 1, n).copy(),
                xnorm=o[4 * n + ns:5 * n + ns].copy(), min=o[-8:-4].copy(), max=o[-4:].copy(), stderr=err)
