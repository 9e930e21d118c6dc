"""Developer script: what a step of the stepped closed loop (TubeTrackingMPC.open_closed_loop, include/tmpc.h: tmpc_mc_open) costs
beside the per-step device loop the library runs on its own, run_closed_loop(fused="off") -- the same solves and state machines;
the difference is the caller's plant kernels and an event each way per step.

    python scripts/gpu_stepped.py [B] [T] [N]          default 4096 100 10 (and the small batch 200 x 100 at N = 20)

Per set-up: three interleaved runs per side, medians and ranges.  The session's clock starts AFTER open_closed_loop (events, the
pinned block, uploads and a synchronisation: one-off, printed on its own) and stops with the statistics on the host; the run's
covers the whole call, its uploads included.  Then the plant's kernels alone on the stream (T steps, events around them), and the
remainder = session steps - run - plant."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
import common                                                     # noqa: E402
from LinearMPCOverNetworks import montecarlo                      # noqa: E402

REPS = 3


def med(v):
    v = sorted(v)
    return f"{1e3 * v[len(v) // 2]:8.2f} ms [{1e3 * v[0]:.2f} .. {1e3 * v[-1]:.2f}]"


def measure(B, T, N):
    mpc, w = common.make_mpc("cartpole", N, True, create=True)
    th, ga, wd = montecarlo.draw_realisations(B, T, w["w_bound"], seed=99)
    pl = np.full(B, 0.3)
    ref = np.where(np.arange(T) < T // 2, 0.5, -0.5)
    dev = torch.device("cuda", 0)
    A = torch.as_tensor(np.asarray(w["A"], dtype=np.float64), device=dev)
    Bm = torch.as_tensor(np.asarray(w["B"], dtype=np.float64), device=dev)
    wt = torch.as_tensor(np.ascontiguousarray(wd.transpose(1, 0, 2)), device=dev)
    stream = torch.cuda.Stream(device=dev)

    def plant(x, u, t):
        return torch.addmm(wt[t], x, A.T).addmm_(u, Bm.T)          # x A' + u B' + w_t: two kernels

    def session(warm):
        with torch.cuda.stream(stream):
            x = torch.zeros((B, 4), dtype=torch.float64, device=dev)
            t0 = time.perf_counter()
            s = mpc.open_closed_loop(pl, ref, th, ga, warm_start=warm)
            t1 = time.perf_counter()
            for t in range(T):
                x = plant(x, s.step(x), t)
            out = s.close()
            out["x_final"] = x.cpu().numpy()
            return time.perf_counter() - t1, t1 - t0, out

    def run(warm):
        t0 = time.perf_counter()
        out = mpc.run_closed_loop(pl, ref, th, ga, wd, warm_start=warm, fused="off")
        return time.perf_counter() - t0, out

    def plant_alone():
        with torch.cuda.stream(stream):
            x = torch.zeros((B, 4), dtype=torch.float64, device=dev)
            u = torch.zeros((B, 1), dtype=torch.float64, device=dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for t in range(T):
                x = plant(x, u, t)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3

    run(False), session(False), plant_alone()                     # warm-up: allocations, kernel loading
    for warm in (False, True):
        ts, to, tr, tp = [], [], [], []
        for _ in range(REPS):                                      # interleaved
            a, o, so = session(warm)
            b, ro = run(warm)
            ts.append(a), to.append(o), tr.append(b), tp.append(plant_alone())
        same = np.max(np.abs(so["x_final"] - ro["x_final"]))
        rem = sorted(a - b - c for a, b, c in zip(ts, tr, tp))
        print(f"cart-pole N = {N}, B = {B}, T = {T}, warm start {'on ' if warm else 'off'} (iterations per solve {so['iters_mean']:.2f} / {ro['iters_mean']:.2f}; "
              f"max |x_final session - run| {same:.1e})")
        print(f"   open_closed_loop (one-off, not in the session)  {med(to)}")
        print(f"   session, torch plant on the caller's stream  {med(ts)} = {B * T / sorted(ts)[REPS // 2]:.3e} steps/s, {1e6 * sorted(ts)[REPS // 2] / T:.1f} us per step")
        print(f"   run_closed_loop(fused='off')                 {med(tr)} = {B * T / sorted(tr)[REPS // 2]:.3e} steps/s, {1e6 * sorted(tr)[REPS // 2] / T:.1f} us per step")
        print(f"   the plant's kernels alone ({T} steps)         {med(tp)}")
        print(f"   remainder (session - run - plant)            {1e3 * rem[REPS // 2]:8.2f} ms [{1e3 * rem[0]:.2f} .. {1e3 * rem[-1]:.2f}] = "
              f"{1e6 * rem[REPS // 2] / T:.1f} us per step", flush=True)
    mpc._close()


if __name__ == "__main__":
    if len(sys.argv) > 1:
        measure(int(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 100, int(sys.argv[3]) if len(sys.argv) > 3 else 10)
    else:
        measure(4096, 100, 10)
        measure(200, 100, 20)             # the reference's experiment size: a step is launch latency
