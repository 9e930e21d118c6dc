"""The device closed loops through the explicit law next to the loops that solve every step (tmpc_mc_set_law).

    python scripts/gpu_law_loop.py [--reps 30] [--out profiles/NAME.txt] [--quick]

Cart-pole N = 10, 4096 trajectories x 100 steps, and N = 20, 200 x 250 (the reference's own experiment size); realisations drawn on the
device, so that a call uploads nothing.  Each loop is repeated `reps` times after three warm-up calls.  Two clocks per call:
  dev  -- HIP events on the handle's stream (tmpc_kernel_ms_total): around the ONE launch of a fused loop, state machines included; in a
          per-step loop around the law's and the solve launches of every step, summed -- the state-machine launches lie outside;
  wall -- the host's clock around the call, everything included (the steps/s figure is B T / median wall).
Per horizon, cold and warm: the loops that solve every step (fused, per step: the references), then through the table of a pilot sweep
(its first --pilot trajectories) at max_tries 1, 4, 16 and all and, with all, after tmpc_law_reorder, fused and per step, and through an empty table (the cost of the law phase on a loop that never hits).
Before and after the reorder, with every candidate allowed: the search with hops (tmpc_law_set_hops) at max_hops 0, 4, 16 and 64, the four
settings INTERLEAVED call by call, with the chains' counters of the timed calls."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import common                                                                   # noqa: E402
from LinearMPCOverNetworks import _native                                        # noqa: E402


def timed(mpc, reps, **kw):
    h = mpc._handle
    dev, wall, out = [], [], None
    for i in range(reps + 3):
        _native.kernel_ms_total(h, reset=True)
        t0 = time.perf_counter()
        out = mpc.run_closed_loop(**kw)
        dt = time.perf_counter() - t0
        ms, _ = _native.kernel_ms_total(h, reset=True)
        if i >= 3:
            dev.append(ms)
            wall.append(1e3 * dt)
    return np.asarray(dev), np.asarray(wall), out


def timed_hops(mpc, table, reps, hops, **kw):
    """One call per setting of max_hops in turn, reps + 3 rounds (the first three are warm-up) -> per setting (dev, wall, out, counters of the timed calls)."""
    h = mpc._handle
    got = {mh: ([], [], None, np.zeros(6, np.int64)) for mh in hops}
    for i in range(reps + 3):
        for mh in hops:
            table.set_hops(mh)
            table.hop_stats(clear=True)
            _native.kernel_ms_total(h, reset=True)
            t0 = time.perf_counter()
            out = mpc.run_closed_loop(**kw)
            dt = time.perf_counter() - t0
            ms, _ = _native.kernel_ms_total(h, reset=True)
            if i >= 3:
                dev, wall, _, st = got[mh]
                dev.append(ms)
                wall.append(1e3 * dt)
                st += np.array(list(table.hop_stats().values()), np.int64)
                got[mh] = (dev, wall, out, st)
    table.set_hops(0)
    return {mh: (np.asarray(d), np.asarray(w_), o, st) for mh, (d, w_, o, st) in got.items()}


def measure(N, B, T, reps, lines, n_pilot):
    mpc, w = common.make_mpc("cartpole", N, True, create=True)
    law = mpc.explicit_law()
    base = dict(p_loss=(np.arange(B) % 10) / 10.0, ref=np.where(np.arange(T) < T // 2, 0.5, -0.3), device_rng=(11, 0, w["w_bound"]))

    def say(name, dev, wall, out, ref_dev=None, hop=None):
        steps = B * T
        extra = ""
        if "law_hits" in out:
            extra = f"  hit rate {out['law_hits'].sum() / steps:6.1%}  mean tries {out['law_tries'].sum() / steps:6.2f}"
        if ref_dev is not None:
            extra += f"  outside the reference's spread on the faster side: {bool(dev.max() < ref_dev.min())}"
        if hop is not None and hop[1] > 0:
            calls, hits, chains = len(dev), max(1, int(out["law_hits"].sum())), steps * len(dev)
            extra += (f"  chain hits {hop[0] / calls / hits:6.1%} of hits, hops per chain hit {(hop[1] - chains) / max(1, hop[0]):5.2f}, chains ended: absent "
                      f"{hop[2] / chains:6.1%} cap {hop[3] / chains:6.1%} two-cycle {hop[4] / chains:6.1%} parameter row {hop[5] / chains:6.1%}")
        lines.append(f"N = {N:2d} B = {B:4d} T = {T:3d}  {name:48s} dev min {dev.min():9.3f} median {np.median(dev):9.3f} max {dev.max():9.3f} ms   "
                     f"wall median {np.median(wall):9.3f} ms   {steps / (1e-3 * np.median(wall)):12.0f} MPC steps/s{extra}")
        print(lines[-1], flush=True)

    def hop_rows(tag, what, warm, refs):
        """The table as it stands at max_hops 0 / 4 / 16 / 64, the four settings interleaved, fused and per step."""
        for fused in ("on", "off"):
            for mh, (dev, wall, out, st) in timed_hops(mpc, law, reps, (0, 4, 16, 64), fused=fused, warm_start=warm, law=True, **base).items():
                say(f"{tag}, {what}, max_hops {mh:2d}, fused {fused}", dev, wall, out, refs[fused], st)

    for warm in (False, True):
        tag = "warm" if warm else "cold"
        refs = {}
        for fused in ("on", "off"):
            dev, wall, out = timed(mpc, reps, fused=fused, warm_start=warm, **base)
            refs[fused] = dev
            say(f"{tag}, solved every step, fused {fused}", dev, wall, out)
        law.clear()
        for fused in ("on", "off"):
            dev, wall, out = timed(mpc, reps, fused=fused, warm_start=warm, law=True, **base)
            say(f"{tag}, empty table, fused {fused}", dev, wall, out, refs[fused])
        # the pilot: the first `n_pilot` trajectories of the sweep (the draws are keyed by the trajectory's index), through the empty table
        Bp = min(B, n_pilot)
        pilot = mpc.run_closed_loop(fused="on", warm_start=warm, law=dict(miss_capacity=Bp * T), **dict(base, p_loss=base["p_loss"][:Bp]))
        _, n_new = law.learn_from_misses(pilot)
        lines.append(f"N = {N:2d} B = {B:4d} T = {T:3d}  {tag}: {n_new} regions learnt from the {pilot['law_misses']()['n_total']} steps of a pilot sweep of {Bp} trajectories")
        print(lines[-1], flush=True)
        for mt in (1, 4, 16, 0):
            for fused in ("on", "off"):
                dev, wall, out = timed(mpc, reps, fused=fused, warm_start=warm, law=mt if mt else True, **base)
                say(f"{tag}, pilot's table, max_tries {mt if mt else 'all'}, fused {fused}", dev, wall, out, refs[fused])
        hop_rows(tag, "pilot's table", warm, refs)
        # the search order by the hit counters of the sweeps so far (tmpc_law_reorder): the walk behind a failed hint gets shorter
        law.reorder()
        for fused in ("on", "off"):
            dev, wall, out = timed(mpc, reps, fused=fused, warm_start=warm, law=True, **base)
            say(f"{tag}, pilot's table reordered, all, fused {fused}", dev, wall, out, refs[fused])
        hop_rows(tag, "reordered", warm, refs)
    mpc._close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pilot", type=int, default=256, help="trajectories of the pilot sweep the table is learnt from")
    ap.add_argument("--quick", action="store_true", help="small loops, three calls each: does the script run?")
    args = ap.parse_args()
    lines = []
    for N, B, T in (((10, 64, 8), (20, 8, 6)) if args.quick else ((10, 4096, 100), (20, 200, 250))):
        measure(N, B, T, 3 if args.quick else args.reps, lines, args.pilot)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
