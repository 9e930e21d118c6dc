"""TEST INFRASTRUCTURE: drives tests/wavesim/senssim_* (the sensitivity kernel of csrc/tmpc_sens.hip on the host execution model;
the file format is described in senssim_main.cpp)."""

import numpy as np

from hostsim import run_files


def run(binary, H, F, G, g0, Ebar, Y, Yp, P, Z, status=None, act_tol=1e-7, mode="jacobian", ybar=None, env=None):
    """One launch on raw condensed data, arguments and result as LinearMPCOverNetworks.sensitivity.qp_sensitivity (plus stderr).  The
    instance-independent products H^-1, W = G H^-1, H^-1 F are formed here the way the numpy twin forms them."""
    H, F, G, g0, Ebar, Y, Yp = (np.asarray(a, dtype=np.float64) for a in (H, F, G, g0, Ebar, Y, Yp))
    nv, npar = F.shape
    nc, ny = g0.shape[0], Y.shape[0]
    P, Z = np.asarray(P, dtype=np.float64).reshape(-1, npar), np.asarray(Z, dtype=np.float64).reshape(-1, nv)
    B, vjp = P.shape[0], mode == "vjp"
    Hinv = np.linalg.inv(0.5 * (H + H.T))
    Hinv = 0.5 * (Hinv + Hinv.T)
    st = np.zeros(B, np.int32) if status is None else np.asarray(status, dtype=np.int32)
    payload = [np.array([nv, nc, npar, ny, B, int(vjp)], dtype=np.int64), np.array([act_tol]), H, Hinv, F, Hinv @ F, G.reshape(nc, nv), G.reshape(nc, nv) @ Hinv,
               g0, Ebar.reshape(nc, npar), Y, Yp, P, Z, st] + ([np.asarray(ybar, dtype=np.float64).reshape(B, ny)] if vjp else [])
    raw, err = run_files(binary, "run", payload, env)
    nout, nw = (npar if vjp else ny * npar), (nc + 31) // 32
    out = np.frombuffer(raw, dtype=np.float64, count=B * nout).reshape((B, npar) if vjp else (B, ny, npar)).copy()
    off = 8 * B * nout
    flag = np.frombuffer(raw, dtype=np.int32, count=B, offset=off).copy()
    nact = np.frombuffer(raw, dtype=np.int32, count=B, offset=off + 4 * B).copy()
    active = np.frombuffer(raw, dtype=np.uint32, count=B * nw, offset=off + 8 * B).reshape(B, nw).copy()
    assert off + 8 * B + 4 * B * nw == len(raw), (off, len(raw))
    return dict(out=out, flag=flag, n_active=nact, active=active, stderr=err)
