"""Device time of the weight-gradient call next to the plain vector-Jacobian call and the solve (HIP events of the handle:
tmpc_last_kernel_ms, which for tmpc_sens_vjp_weights_device spans the sensitivity launch and the two reduction kernels, not the copy
of the results to the host).

    python scripts/gpu_sens_weights.py [--reps 30] [--out profiles/NAME.txt] [--parent /path/to/the/parent's/libtmpc_hip.so]

Per 4096 cart-pole N = 10 instances and per 1024 config-5 instances (synthetic nx 12, nu 4, N 30): solve, tmpc_sens_vjp_device and
tmpc_sens_vjp_weights_device through the device-pointer entries, each `reps` times after three warm-up calls; printed: minimum, median,
maximum.  --parent: tmpc_sens_vjp_device also against another build of the library (the kernel gained two pointer tests), parent and
tree alternating, three fresh processes a side; the tree's median of medians may exceed the parent's by no more than the parent's own
spread across its runs (the rule of DESIGN.md 7k)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(label, mpc, X, R, reps, lines, result):
    import torch
    from LinearMPCOverNetworks import _native
    h = mpc._handle
    B = len(X)
    nx, nu, N = h.nx, h.nu, h.N
    ny = N * nu + 2 * nx + nu
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x, r = dev(X), dev(R)
    u = torch.empty((B, N, nu), dtype=torch.float64, device="cuda")
    x0 = torch.empty((B, nx), dtype=torch.float64, device="cuda")
    ss = torch.empty((B, nx + nu), dtype=torch.float64, device="cuda")
    st = torch.empty(B, dtype=torch.int32, device="cuda")
    it = torch.empty(B, dtype=torch.int32, device="cuda")
    ybar = dev(np.random.default_rng(0).standard_normal((B, ny)))
    pbar = torch.empty((B, 2 * nx), dtype=torch.float64, device="cuda")
    flag = torch.empty(B, dtype=torch.int32, device="cuda")
    nact = torch.empty(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sens = (h, B, x.data_ptr(), r.data_ptr(), None, u.data_ptr(), x0.data_ptr(), ss.data_ptr(), st.data_ptr(), 0.0, ybar.data_ptr(), pbar.data_ptr(),
            flag.data_ptr(), nact.data_ptr())
    calls = {"solve": lambda: _native.solve_batch_device(h, B, x.data_ptr(), r.data_ptr(), None, u.data_ptr(), x0.data_ptr(), ss.data_ptr(), None, st.data_ptr(), it.data_ptr()),
             "vjp": lambda: _native.sens_vjp_device(*sens)}
    if hasattr(_native.lib(), "tmpc_sens_vjp_weights_device"):          # (an older build loaded through TMPC_LIB has none)
        calls["vjp_weights"] = lambda: _native.sens_vjp_weights_device(*sens)
    for name, call in calls.items():
        ms = []
        for i in range(reps + 3):
            call()
            t = _native.last_kernel_ms(h)
            _native.synchronize(h)
            if i >= 3:
                ms.append(t)
        ms = np.asarray(ms)
        result[f"{label}/{name}"] = [float(ms.min()), float(np.median(ms)), float(ms.max())]
        lines.append(f"{label:28s} B = {B:5d}  {name:11s} min {ms.min():8.4f}  median {np.median(ms):8.4f}  max {ms.max():8.4f} ms   ({reps} calls)")
        print(lines[-1], flush=True)


def run(reps):
    import common
    lines, result = [], {}
    S = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
    XR = S[np.arange(4096) % len(S)]
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True)
    measure("cart-pole N = 10 (nv 11)", mpc, XR[:, :4], XR[:, 4:], reps, lines, result)
    mpc._close()
    mpc, _ = common.make_mpc("synthetic", 30, True, create=True)
    rng = np.random.default_rng(1)
    box = np.asarray(mpc._Xc.b[:12], dtype=np.float64)         # interior states and position references (tests/shape_cases.tracking_states)
    X = rng.uniform(-0.6, 0.6, (1024, 12)) * box
    R = np.c_[rng.uniform(-0.8, 0.8, 1024) * box[0], np.zeros((1024, 11))]
    measure("config 5 (nx 12 nu 4 N 30)", mpc, X, R, reps, lines, result)
    mpc._close()
    return lines, result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--json", action="store_true", help="(the A/B's children) one JSON line with the figures")
    args = ap.parse_args()
    lines, result = run(args.reps)
    if args.json:
        print(json.dumps(result), flush=True)
        return 0
    if args.parent:
        sides = {"parent": os.path.abspath(args.parent), "tree": ""}
        got = {s: [] for s in sides}
        lines.append(f"tmpc_sens_vjp_device, parent {sides['parent']} against the tree, fresh processes, alternating; median of {args.reps} calls per run, ms")
        for rnd in range(3):
            for side in (list(sides) if rnd % 2 == 0 else list(sides)[::-1]):
                env = dict(os.environ)
                env.pop("TMPC_LIB", None)
                if sides[side]:
                    env["TMPC_LIB"] = sides[side]
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--json"], env=env, capture_output=True, text=True, timeout=300)
                if p.returncode != 0:             # (a fault or an abort on one side: nothing more is started on the card)
                    print(f"{side} run {rnd + 1} FAILED rc {p.returncode}\n{p.stderr[-3000:]}", flush=True)
                    return 1
                got[side].append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]))
        for key in [k for k in got["tree"][0] if k.endswith("/vjp")]:
            par = np.array([g[key][1] for g in got["parent"]])
            tre = np.array([g[key][1] for g in got["tree"]])
            spread = par.max() - par.min()
            ok = np.median(tre) <= np.median(par) + spread
            lines.append(f"{key:40s} parent {np.array2string(par, precision=4)} tree {np.array2string(tre, precision=4)}  medians {np.median(par):.4f} / {np.median(tre):.4f}"
                         f"  parent's spread {spread:.4f}  {'within' if ok else 'EXCEEDS'}")
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
