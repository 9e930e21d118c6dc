"""TEST INFRASTRUCTURE: drives tests/wavesim/plantsim_* (the W estimate's rollout with a plant per trajectory on the host execution
model; the file formats are described in plantsim_main.cpp)."""

import numpy as np

from hostsim import run_files


def run_rollout(binary, Acl, K, par7, par_traj, T, substeps=10, x0=None, box=None, n_traj=None, seed=0, first=0, env=None):
    """west_case.run_rollout with a cart-pole per trajectory, par_traj (n, 7); par7 is the call's own row, which no lane may use.
    Returns dict(x0_used (n, 4), samples (4, T - 1, n), xnorm (n), min (4), max (4), stderr)."""
    draw = x0 is None
    n = int(n_traj) if draw else np.asarray(x0).reshape(-1, 4).shape[0]
    lo, hi = box if draw else (np.zeros(4), np.zeros(4))
    payload = [np.asarray(Acl, dtype=np.float64), np.asarray(K, dtype=np.float64).reshape(4), np.asarray(par7, dtype=np.float64),
               np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64),
               np.array([substeps, T, int(draw), n, first, seed], dtype=np.int64)]
    if not draw:
        payload.append(np.asarray(x0, dtype=np.float64).reshape(-1, 4))
    payload.append(np.asarray(par_traj, dtype=np.float64).reshape(n, 7))
    raw, err = run_files(binary, "rollout", payload, env)
    o = np.frombuffer(raw, dtype=np.float64)
    ns = 4 * (T - 1) * n
    return dict(x0_used=o[:4 * n].reshape(n, 4).copy(), samples=o[4 * n:4 * n + ns].reshape(4, T - 1, n).copy(),
                xnorm=o[4 * n + ns:5 * n + ns].copy(), min=o[-8:-4].copy(), max=o[-4:].copy(), stderr=err)
