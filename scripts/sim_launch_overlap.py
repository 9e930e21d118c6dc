"""A discrete-event model of how the card's CUs go to overlapped solve launches (DESIGN.md 5.1 "Between launches"): CPU only, numpy only, a
MODEL and not a measurement -- DESIGN.md sets what it says beside what the A/Bs measured.

  python scripts/sim_launch_overlap.py [--ticks profiles/r16_bench_solve_ticks.txt] [--calls 200] [--cus 256]

The model
  * n_cu CUs; a launch is `grid` workgroups of WPB = 8 waves, one workgroup per CU (the LDS admits no second one).
  * A workgroup stages the model (t_stage), then each of its waves solves its first item and draws further ones from the launch's counter until
    the counter has run dry; the CU is free when the last of the eight waves has left.
  * The first `core` workgroups take static first items, the counter serves the rest (core = grid: today's launch).  A surplus workgroup of an
    elastic launch looks at the number of younger calls enqueued beside its launch when it starts: with lanes - 1 or more it leaves after
    t_yield, else it joins with a grouped draw.  The host is taken to be far ahead of the card (bench.py enqueues its 200 calls in a few
    milliseconds): a call's followers are the calls behind it in the burst.
  * A launch on a stream waits for the one before it on that stream; streams may share a hardware queue, which serialises them the same way.
  * Free CUs go to the oldest eligible launch that still has workgroups to place.
  * Instance costs: the measured per-instance ticks of one bench batch (--ticks, 10 ns each), drawn in a fresh random order per call; without the
    file, 35 + 8.5 * iters microseconds with iters ~ N(10.9, 1.7) clipped to 8 ... 19 and 1.2 % trivial instances."""
import argparse
import heapq
import os

import numpy as np

WPB = 8


def instance_costs(rng, ticks, n):
    if ticks is not None:
        return rng.permutation(ticks)[:n] if n <= len(ticks) else rng.choice(ticks, n)
    it = np.clip(rng.normal(10.9, 1.7, n), 8, 19)
    c = 35.0 + 8.5 * it
    c[rng.random(n) < 0.012] = 6.0
    return c


def simulate(calls, streams, grid, core, lanes_for_yield, B, n_cu, rng, ticks, queue_of=None, t_stage=4.0, t_yield=3.0, wgs_per_cu=1, wpb=WPB):
    """`calls` launches of B items in rotation over `streams` streams -> (makespan in us, share of wave-slot time in use)"""
    queue_of = queue_of or list(range(streams))
    cost = [instance_costs(rng, ticks, B) for _ in range(calls)]
    nxt = [0] * calls                      # counter: items handed out behind the static ones
    placed = [0] * calls                   # workgroups placed
    alive = [0] * calls                    # workgroups on the card
    done = [False] * calls
    static = min(core, grid) * wpb
    # a launch is eligible when every earlier launch of its hardware queue has finished
    prev = [None] * calls
    last_on_queue = {}
    for k in range(calls):
        q = queue_of[k % streams]
        prev[k] = last_on_queue.get(q)
        last_on_queue[q] = k
    free = n_cu * wgs_per_cu
    events = []                            # (time, seq, kind, call, waves left in the workgroup [a one-element list])
    seq = 0
    busy = 0.0
    t = 0.0

    def take(k, w):
        """next item of a wave of launch k (w: its first item or None) -> cost or None"""
        if w is not None:
            return cost[k][w] if w < B else None
        i = static + nxt[k]
        if i >= B:
            return None
        nxt[k] += 1
        return cost[k][i]

    def place(now):
        nonlocal free, seq, busy
        while free > 0:
            k = next((j for j in range(calls) if not done[j] and placed[j] < grid and (prev[j] is None or done[prev[j]])), None)
            if k is None:
                return
            wg = placed[k]
            placed[k] += 1
            free -= 1
            alive[k] += 1
            if wg >= core:                                     # surplus workgroup of an elastic launch
                followers = calls - 1 - k
                if followers >= lanes_for_yield - 1:
                    heapq.heappush(events, (now + t_yield, seq, 1, k, None)); seq += 1
                    continue
                first = [static + nxt[k] + w for w in range(wpb)]
                nxt[k] += wpb
            else:
                first = [wg * wpb + w for w in range(wpb)] if B >= grid * wpb else [w * grid + wg for w in range(wpb)]
            left = [wpb]
            for w in first:
                c = take(k, w)
                if c is None:
                    left[0] -= 1
                else:
                    busy += c
                    heapq.heappush(events, (now + t_stage + c, seq, 0, k, left)); seq += 1
            if left[0] == 0:
                heapq.heappush(events, (now + t_stage, seq, 1, k, None)); seq += 1

    place(0.0)
    while events:
        t, _, kind, k, left = heapq.heappop(events)
        if kind == 0:
            c = take(k, None)
            if c is not None:
                busy += c
                heapq.heappush(events, (t + c, seq, 0, k, left)); seq += 1
                continue
            left[0] -= 1
            if left[0] > 0:
                continue
        # the workgroup leaves: its CU is free
        free += 1
        alive[k] -= 1
        if alive[k] == 0 and placed[k] == grid:
            done[k] = True
        place(t)
    return t, busy / (n_cu * wgs_per_cu * wpb * t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r16_bench_solve_ticks.txt"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    ticks = None
    if os.path.exists(a.ticks):
        ticks = np.loadtxt(a.ticks)[:, 0] / 100.0          # 10 ns ticks -> us
        print(f"instance costs: {a.ticks}: {len(ticks)} instances, mean {ticks.mean():.1f} us, min {ticks.min():.1f}, max {ticks.max():.1f}")
    else:
        print("instance costs: 35 + 8.5 iters us (no tick file)")
    n, B = a.cus, a.batch
    third, quarter = -(-n // 2), -(-n // 3)
    rows = [
        ("one lane, grid n_cu", dict(streams=1, grid=n, core=n, lanes_for_yield=1)),
        ("two lanes, grid n_cu (the parent)", dict(streams=2, grid=n, core=n, lanes_for_yield=2)),
        ("three lanes, fixed grid n_cu/2", dict(streams=3, grid=third, core=third, lanes_for_yield=3)),
        ("four lanes, fixed grid n_cu/3", dict(streams=4, grid=quarter, core=quarter, lanes_for_yield=4)),
        ("four lanes, grid n_cu, not elastic", dict(streams=4, grid=n, core=n, lanes_for_yield=4)),
        ("three lanes, elastic", dict(streams=3, grid=n, core=third, lanes_for_yield=3)),
        ("four lanes, elastic", dict(streams=4, grid=n, core=quarter, lanes_for_yield=4)),
        ("four lanes, elastic, two of them on one hardware queue", dict(streams=4, grid=n, core=quarter, lanes_for_yield=4, queue_of=[0, 1, 2, 2])),
    ]
    print(f"\n{a.calls} calls of {B} on {n} CUs: share of wave-slot time in use, wall time against the parent's")
    base = None
    for name, kw in rows:
        t, u = simulate(a.calls, B=B, n_cu=n, rng=np.random.default_rng(a.seed), ticks=ticks, **kw)
        if name.startswith("two lanes"):
            base = t
        rel = f"{t / base:.3f}" if base else "  -  "
        print(f"  {name:58s} {u:.3f}   {t / a.calls:7.1f} us per call   {rel}")
    t, u = simulate(max(a.calls // 16, 4), streams=1, grid=n, core=n, lanes_for_yield=1, B=16 * B, n_cu=n, rng=np.random.default_rng(a.seed), ticks=ticks)
    print(f"  {'B = 16 x batch, one lane':58s} {u:.3f}   {t / max(a.calls // 16, 4) / 16:7.1f} us per {B}")
    print("\nbursts: wall time against the parent's (two lanes, grid n_cu)")
    print("  calls   fixed n_cu/3, four lanes   elastic, four lanes   elastic, three lanes")
    for k in (1, 2, 3, 4, 8, 16, 200):
        r = []
        for kw in (dict(streams=2, grid=n, core=n, lanes_for_yield=2), dict(streams=4, grid=quarter, core=quarter, lanes_for_yield=4),
                   dict(streams=4, grid=n, core=quarter, lanes_for_yield=4), dict(streams=3, grid=n, core=third, lanes_for_yield=3)):
            r.append(np.mean([simulate(k, B=B, n_cu=n, rng=np.random.default_rng(a.seed + s), ticks=ticks, **kw)[0] for s in range(3 if k < 100 else 1)]))
        print(f"  {k:5d}   {r[1] / r[0]:24.3f}   {r[2] / r[0]:19.3f}   {r[3] / r[0]:20.3f}")


if __name__ == "__main__":
    main()
