"""TEST INFRASTRUCTURE: drives tests/wavesim/lawsim_* (the explicit-law kernel of csrc/tmpc_law.hip on the host execution model; the
file format is described in lawsim_main.cpp)."""

import numpy as np

from hostsim import run_files


def pack_table(table, npar, ny, nrow):
    """The regions of LinearMPCOverNetworks.explicit_law.region_law in the layout tmpc_law.cpp uploads: S [R][np + 1][nrowp] (padding rows
    0 p + 1; a None entry holds no p: 0 p - 1), K [R][np + 1][ny]."""
    nrowp = (nrow + 63) // 64 * 64
    S, K = np.zeros((len(table), npar + 1, nrowp)), np.zeros((len(table), npar + 1, ny))
    for r, t in enumerate(table):
        if t is None:
            S[r, npar] = -1.0
            continue
        S[r, :npar, :nrow], S[r, npar, :nrow], S[r, npar, nrow:] = t["S"].T, t["s"], 1.0
        K[r, :npar], K[r, npar] = t["Ky"].T, t["ky"]
    return S, K


def run(binary, table, P, hint=None, order=None, max_tries=0, env=None):
    """One launch; arguments as LinearMPCOverNetworks.explicit_law.locate -> dict(y, region, tries, hits, stderr)."""
    first = next(t for t in table if t is not None)
    (ny, npar), nrow = first["Ky"].shape, first["s"].shape[0]
    P = np.asarray(P, dtype=np.float64).reshape(-1, npar)
    B, R = P.shape[0], len(table)
    order = np.arange(R, dtype=np.int32) if order is None else np.asarray(order, dtype=np.int32).reshape(-1)
    S, K = pack_table(table, npar, ny, nrow)
    payload = [np.array([npar, ny, nrow, R, len(order), B, max_tries, int(hint is not None)], dtype=np.int64), S, K, order, P]
    if hint is not None:
        payload.append(np.ascontiguousarray(np.broadcast_to(np.asarray(hint, dtype=np.int32).reshape(-1), (B,))))
    raw, err = run_files(binary, "run", payload, env)
    y = np.frombuffer(raw, dtype=np.float64, count=B * ny).reshape(B, ny).copy()
    off = 8 * B * ny
    region = np.frombuffer(raw, dtype=np.int32, count=B, offset=off).copy()
    tries = np.frombuffer(raw, dtype=np.int32, count=B, offset=off + 4 * B).copy()
    hits = np.frombuffer(raw, dtype=np.uint64, count=R, offset=off + 8 * B).copy()
    assert off + 8 * B + 8 * R == len(raw), (off, len(raw))
    return dict(y=y, region=region, tries=tries, hits=hits, stderr=err)
