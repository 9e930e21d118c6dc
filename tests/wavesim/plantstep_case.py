"""TEST INFRASTRUCTURE: drives tests/wavesim/plantstep_* (the plant kernels of csrc/tmpc_plant.hip on the host execution model;
the file format is described in plantstep_main.cpp)."""

import numpy as np

from hostsim import run_files

KIND = {"linear": 0, "cartpole": 1}         # include/tmpc.h: TMPC_PLANT_*


def run_step(binary, family, x, u, w=None, philox=None, hold=None, err2_phys=None, ref_t=0.0, ref_tab=None, ref_id=None, env=None):
    """One launch of the plant kernel for `family` (a montecarlo.PlantFamily) on x (B, nx), u (B, nu).  w (B, nx): the disturbance as an array;
    philox = (t, seed, first, w_bound): the device generator's; neither: none.  hold (B,) bytes; err2_phys (B,): the accumulator going in,
    with ref_t or ref_tab (K, ref_T, nx) + ref_id (B,) and the step t of philox (or 0).  Returns dict(x_plus (B, nx)[, err2_phys (B,)], stderr)."""
    x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
    nb, nx = x.shape
    nu = u.shape[1]
    t, seed, first, w_bound = philox if philox is not None else (0, 0, 0, None)
    wmode = 1 if w is not None else (2 if philox is not None and w_bound is not None else 0)
    phys = 0 if err2_phys is None else (2 if ref_tab is not None else 1)
    tab = None if ref_tab is None else np.asarray(ref_tab, dtype=np.float64).reshape(-1, np.shape(ref_tab)[-2], nx)
    hd = [KIND[family.kind], nx, nu, family.substeps, nb, wmode, t, seed, first, int(hold is not None), phys,
          0 if tab is None else tab.shape[1], 0 if tab is None else tab.shape[0]]
    payload = [np.array(hd, dtype=np.int64), np.asarray(family.models, dtype=np.float64), x, u]
    if wmode == 1:
        payload.append(np.asarray(w, dtype=np.float64).reshape(nb, nx))
    if wmode == 2:
        payload.append(np.asarray(w_bound, dtype=np.float64).reshape(nx))
    if hold is not None:
        payload.append(np.asarray(hold, dtype=np.uint8).reshape(nb))
    if phys:
        payload += [np.asarray(err2_phys, dtype=np.float64).reshape(nb), np.array([ref_t], dtype=np.float64)]
    if phys == 2:
        payload += [tab, np.asarray(ref_id, dtype=np.int32).reshape(nb)]
    raw, err = run_files(binary, "step", payload, env)
    o = np.frombuffer(raw, dtype=np.float64)
    out = dict(x_plus=o[:nb * nx].reshape(nb, nx).copy(), stderr=err)
    if phys:
        out["err2_phys"] = o[nb * nx:nb * nx + nb].copy()
    return out
