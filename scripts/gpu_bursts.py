"""Wall time of short bursts of independent tmpc_solve_batch_device calls (1, 2, 3, 4, 8, 16 calls of 4096 cart-pole QPs, N = 10) for two
builds of lib/libtmpc_hip.so, the protocol of scripts/gpu_lib_ab.py: every run a fresh process, sides alternating, the order reversed from one
round to the next.  A burst starts on an idle handle and ends with tmpc_synchronize; its time is the median of --reps repetitions: a launch that
nobody follows must still spread over the whole card.

  python scripts/gpu_bursts.py --a parent=/path/to/libtmpc_hip.so --b tree= [--runs 3]       (an empty path: the tree's own library)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 4, 8, 16)


def child(reps):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-tracking-mpc-over-lossy-networks_amd")]
    import torch
    from LinearMPCOverNetworks import _native, workloads
    B, nx, nu, N = 4096, 4, 1, 10
    mpc, _ = workloads.make_controller("cartpole", 10, True, device=0)
    h = mpc._handle
    S = np.load(os.path.join(ROOT, "tests", "golden", "cartpole_N10_states.npy"))
    dev = torch.device("cuda:0")
    sets = []
    for k in range(max(SIZES)):
        i = np.random.default_rng(700 + k).integers(0, len(S), B)
        t = [torch.from_numpy(np.ascontiguousarray(S[i, :nx])).to(dev), torch.from_numpy(np.ascontiguousarray(S[i, nx:])).to(dev),
             torch.zeros(B, N, nu, dtype=torch.float64, device=dev), torch.zeros(B, nx, dtype=torch.float64, device=dev),
             torch.zeros(B, nx + nu, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev),
             torch.zeros(B, dtype=torch.int32, device=dev)]
        sets.append(t)
    torch.cuda.synchronize()

    def burst(k):
        for x, r, u, x0, ss, st, it in sets[:k]:
            _native.solve_batch_device(h, B, x.data_ptr(), r.data_ptr(), None, u.data_ptr(), x0.data_ptr(), ss.data_ptr(), None, st.data_ptr(), it.data_ptr())
        _native.synchronize(h)

    for _ in range(8):                       # lanes created, clocks up
        burst(max(SIZES))
    out = {}
    for k in SIZES:
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            burst(k)
            ts.append(time.perf_counter() - t0)
        out[str(k)] = float(np.median(ts) * 1e6)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a")
    ap.add_argument("--b")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.reps)
    sides = [s.split("=", 1) for s in (args.a, args.b)]
    res = {n: [] for n, _ in sides}
    print(f"## bursts of {SIZES} calls of 4096, wall us per burst (median of {args.reps})", flush=True)
    for rnd in range(args.runs):
        for name, lib in (sides if rnd % 2 == 0 else sides[::-1]):
            env = dict(os.environ)
            env.pop("TMPC_LIB", None)
            if lib:
                env["TMPC_LIB"] = os.path.abspath(lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)], env=env, capture_output=True, text=True,
                               timeout=300, cwd=ROOT)
            if p.returncode != 0:
                print(f"{name}_{rnd + 1} FAILED rc {p.returncode}\n{p.stderr[-3000:]}", flush=True)      # (nothing more is started on the card)
                return 1
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            res[name].append(r)
            print(f"{name}_{rnd + 1}  " + "  ".join(f"{k}: {r[str(k)]:8.1f}" for k in SIZES), flush=True)
    (na, _), (nb, _) = sides
    for k in SIZES:
        va, vb = (np.array([r[str(k)] for r in res[n]]) for n in (na, nb))
        apart = va.max() < vb.min() or vb.max() < va.min()
        crit = apart and abs(np.median(vb) - np.median(va)) >= 3 * max(np.ptp(va), np.ptp(vb))
        verdict = "within the criterion" if not crit else ("FASTER" if np.median(vb) < np.median(va) else "SLOWER")
        print(f"burst of {k:2d}: {na} {np.median(va):8.1f} [{va.min():.1f}, {va.max():.1f}]  {nb} {np.median(vb):8.1f} [{vb.min():.1f}, {vb.max():.1f}]  "
              f"{nb}/{na} {np.median(vb) / np.median(va):.4f}  {verdict}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
