"""python scripts/gpu_reference_cost.py -- cost of the full-reference mode: the bench's closed loop (cart-pole N = 10, 4096 x 100, p_loss 0.3) with the legacy reference and
with tables K = 1, 8, B holding the same reference; interleaved repetitions, median [range] of the wall time of run_closed_loop."""
import os, sys, time, json
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "robust-tracking-mpc-over-lossy-networks_amd")]
from LinearMPCOverNetworks import montecarlo, workloads
mpc, w = workloads.make_controller("cartpole", 10, True)
B, T = 4096, 100
th, ga, wd = montecarlo.draw_realisations(B, T, w["w_bound"], seed=99)
pl = np.full(B, 0.3)
ref = np.where(np.arange(T) < T // 2, 0.5, -0.5)
row = np.zeros((T, 4)); row[:, 0] = ref
cases = {"legacy": dict(ref=ref), "K=1": dict(ref=row), "K=8": dict(ref=np.broadcast_to(row, (8, T, 4)).copy(), ref_id=np.arange(B) % 8),
         "K=B": dict(ref=np.broadcast_to(row, (B, T, 4)).copy())}
res = {}
for mode in (None, "off"):
    for warm in (False, True):
        times = {k: [] for k in cases}
        outs = {}
        for rep in range(6):
            for k, kw in cases.items():
                t0 = time.perf_counter()
                outs[k] = mpc.run_closed_loop(pl, kw["ref"], th, ga, wd, warm_start=warm, fused=mode, ref_id=kw.get("ref_id"))
                dt = time.perf_counter() - t0
                if rep:                       # the first round warms up
                    times[k].append(dt)
        same = {k: all(np.array_equal(outs[k][q], outs["legacy"][q]) for q in ("err2", "x_final", "tube_violations", "not_optimal", "iters_sum")) for k in cases}
        for k in cases:
            t = np.array(times[k]) * 1e3
            key = f"fused={mode or 'auto'} warm={warm} {k}"
            res[key] = dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), loop_mode=int(outs[k]["loop_mode"]), same_bytes_as_legacy=bool(same[k]))
            print(key, json.dumps(res[key]), flush=True)
