"""TEST INFRASTRUCTURE: drives tests/wavesim/lawloop_* (the fused closed loop through the explicit law, closed_loop_law of
csrc/tmpc_kernels.hip, on the host execution model; the file formats are described in lawloop_main.cpp and wavesim_main.cpp)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from law_case import pack_table


def run(binary, d, K, K_anc, Z, p_loss, ref, th_u, ga_u, w, table, shape, order=None, max_tries=0, miss_capacity=0, warm=False, env=None, timeout=3600):
    """The loop of run_case.run_loop (plain controller of problem dict `d`) through `table`, a list of explicit_law.region_law dicts (None:
    a region that holds no p; [] with shape = (np, ny, nrow): the empty table).  -> the loop's statistics plus region, hits, tries (B,),
    region_hits (R,), n_total and the miss log x_k, ref, variant."""
    from LinearMPCOverNetworks import _native
    L = _native.lib()
    L.tmpc_debug_dump_layout.argtypes = [C.c_void_p, C.c_int, C.c_char_p]
    h = _native.create(d, -1)
    try:
        with tempfile.TemporaryDirectory() as tmp:
            lay, loop, tab, out = (os.path.join(tmp, n) for n in ("layout.bin", "loop.bin", "table.bin", "out.bin"))
            rc = L.tmpc_debug_dump_layout(h.ptr, 0, lay.encode())
            if rc != 0:
                raise RuntimeError(f"tmpc_debug_dump_layout failed: {rc}")
            c = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))
            th_u, ga_u, w = c(th_u), c(ga_u), c(w)
            B, T = th_u.shape
            nx, nu = h.nx, h.nu
            HZ = np.zeros((0, nx)) if Z is None else c(Z.A)
            hZ = np.zeros(0) if Z is None else c(Z.b)
            with open(loop, "wb") as f:
                np.array([B, T, nx, nu, HZ.shape[0], 0, 0, int(bool(warm))], dtype=np.int64).tofile(f)
                for a in (np.asarray(d["A"]), np.asarray(d["B"]), K, K_anc, HZ, hZ, p_loss, ref, th_u, ga_u, w, np.zeros((B, nx))):
                    c(a).tofile(f)
            npar, ny, nrow = shape
            R = len(table)
            order = np.arange(R, dtype=np.int32) if order is None else np.asarray(order, dtype=np.int32).reshape(-1)
            S, Kt = pack_table(table, npar, ny, nrow)
            with open(tab, "wb") as f:
                np.array([npar, ny, nrow, R, len(order), max_tries, miss_capacity], dtype=np.int64).tofile(f)
                for a in (S, Kt):
                    c(a).tofile(f)
                np.ascontiguousarray(order).tofile(f)
            res = subprocess.run([binary, lay, loop, tab, out], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})))
            if res.returncode != 0:
                raise RuntimeError(f"{os.path.basename(binary)} failed ({res.returncode}):\n{res.stderr[-8000:]}")
            raw = open(out, "rb").read()
    finally:
        _native.destroy(h)
    off = 0

    def take(n, dt):
        nonlocal off
        a = np.frombuffer(raw, dtype=dt, count=n, offset=off).copy()
        off += a.nbytes
        return a
    o = dict(err2=take(B, np.float64), x_final=take(B * nx, np.float64).reshape(B, nx), consistent=take(B, np.float64), tube_violations=take(B, np.int32),
             not_optimal=take(B, np.int32), iters_sum=take(B, np.int32), region=take(B, np.int32), hits=take(B, np.int32), tries=take(B, np.int64),
             region_hits=take(R, np.uint64))
    o["n_total"] = int(take(1, np.uint64)[0])
    kept = min(o["n_total"], miss_capacity)
    P = take(kept * npar, np.float64).reshape(kept, npar)
    o["x_k"], o["ref"], o["variant"] = P[:, :nx], P[:, nx:], take(kept, np.uint8)
    assert off == len(raw), (off, len(raw))
    o["tracking_error"] = np.sqrt(o["err2"]) / T
    o["stderr"] = res.stderr
    return o
