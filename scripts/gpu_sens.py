"""Device time of the sensitivity calls next to the solve they differentiate (HIP events on the handle's stream: tmpc_last_kernel_ms).

    python scripts/gpu_sens.py [--reps 30] [--out profiles/NAME.txt]

Per 4096 cart-pole N = 10 instances (wave kernel) and per 1024 config-5 instances (synthetic nx 12, nu 4, N 30: block kernel): the solve
launch, the Jacobian launch and the vector-Jacobian launch through the device-pointer entries, each repeated `reps` times after three
warm-up calls; printed: minimum, median, maximum.  The solve kernels' code objects are those of the parent commit byte for byte (the
kernel files are untouched), so the solve figure is the parent's, measured in the same session."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import common                                                                   # noqa: E402
from LinearMPCOverNetworks import _native                                        # noqa: E402


def measure(label, mpc, X, R, reps, lines):
    import torch
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
    J = torch.empty((B, ny, 2 * nx), dtype=torch.float64, device="cuda")
    ybar = dev(np.random.default_rng(0).standard_normal((B, ny)))
    pbar = torch.empty((B, 2 * nx), dtype=torch.float64, device="cuda")
    flag = torch.empty(B, dtype=torch.int32, device="cuda")
    nact = torch.empty(B, dtype=torch.int32, device="cuda")
    act = torch.zeros((B, _native.sens_active_words(h)), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    calls = {
        "solve": lambda: _native.solve_batch_device(h, B, x.data_ptr(), r.data_ptr(), None, u.data_ptr(), x0.data_ptr(), ss.data_ptr(), None, st.data_ptr(), it.data_ptr()),
        "jacobian": lambda: _native.sens_jacobian_device(h, B, x.data_ptr(), r.data_ptr(), None, u.data_ptr(), x0.data_ptr(), ss.data_ptr(), st.data_ptr(), 0.0,
                                                         J.data_ptr(), flag.data_ptr(), nact.data_ptr(), act.data_ptr()),
        "vjp": lambda: _native.sens_vjp_device(h, B, x.data_ptr(), r.data_ptr(), None, u.data_ptr(), x0.data_ptr(), ss.data_ptr(), st.data_ptr(), 0.0,
                                               ybar.data_ptr(), pbar.data_ptr(), flag.data_ptr(), nact.data_ptr()),
    }
    for name, call in calls.items():
        ms = []
        for i in range(reps + 3):
            call()
            t = _native.last_kernel_ms(h)
            _native.synchronize(h)
            if i >= 3:
                ms.append(t)
        ms = np.asarray(ms)
        lines.append(f"{label:28s} B = {B:5d}  {name:9s} min {ms.min():8.4f}  median {np.median(ms):8.4f}  max {ms.max():8.4f} ms   ({reps} calls)")
        print(lines[-1], flush=True)
    f = flag.cpu().numpy()
    lines.append(f"{label:28s} flags: {int((f == 0).sum())} clean, {int((f & 1 != 0).sum())} skipped, {int((f & 2 != 0).sum())} dependent, "
                 f"{int((f & 4 != 0).sum())} weak, {int((f & 8 != 0).sum())} not-KKT; mean working set {nact.cpu().numpy().mean():.1f} rows; kernel {_native.kernel_name(h)}")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    S = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
    XR = S[np.arange(4096) % len(S)]
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True)
    measure("cart-pole N = 10 (nv 11)", mpc, XR[:, :4], XR[:, 4:], args.reps, lines)
    mpc._close()
    mpc, _ = common.make_mpc("synthetic", 30, True, create=True)
    rng = np.random.default_rng(1)
    box = np.asarray(mpc._Xc.b[:12], dtype=np.float64)         # interior states and position references (tests/shape_cases.tracking_states)
    X = rng.uniform(-0.6, 0.6, (1024, 12)) * box
    R = np.c_[rng.uniform(-0.8, 0.8, 1024) * box[0], np.zeros((1024, 11))]
    measure("config 5 (nx 12 nu 4 N 30)", mpc, X, R, args.reps, lines)
    mpc._close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
