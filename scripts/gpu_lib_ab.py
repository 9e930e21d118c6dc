"""Interleaved A/B of two builds of lib/libtmpc_hip.so on one card, the protocol of profiles/r13_lane_packing_ab.txt and
profiles/r15_mfma_blocks_ab.txt: every run of bench.py a fresh process, sides alternating (the order reversed from one round to the next),
the first run of every side with --dump-outputs.  Prints one line per run, then per metric of the JSON line the median [min, max] of
every side and the ratio, then the comparison of the two dumps.

  python scripts/gpu_lib_ab.py --a parent=/path/to/libtmpc_hip.so --b blocks= [--runs 3] [--out DIR] -- --gpus 1 --steps 200 --warmup 10
(an empty path: the tree's own library)"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flatten(d, pre=""):
    for k, v in d.items():
        if isinstance(v, dict):
            yield from flatten(v, pre + k + "/")
        elif isinstance(v, (int, float)) and not isinstance(v, bool):
            yield pre + k, float(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True)
    ap.add_argument("--b", required=True)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "ab"))
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--all-metrics", action="store_true")
    ap.add_argument("bench", nargs=argparse.REMAINDER)
    args = ap.parse_args()
    bench_args = [a for a in args.bench if a != "--"]
    sides = [s.split("=", 1) for s in (args.a, args.b)]
    os.makedirs(args.out, exist_ok=True)
    res = {n: [] for n, _ in sides}
    print("## python bench.py " + " ".join(bench_args), flush=True)
    for rnd in range(args.runs):
        for name, lib in (sides if rnd % 2 == 0 else sides[::-1]):
            env = dict(os.environ)
            if lib:
                env["TMPC_LIB"] = os.path.abspath(lib)
            else:
                env.pop("TMPC_LIB", None)
            cmd = [sys.executable, os.path.join(ROOT, "bench.py"), *bench_args]
            if rnd == 0:
                cmd += ["--dump-outputs", os.path.join(args.out, "dump_" + name)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
            if p.returncode != 0:
                # (a fault or an abort on one side: nothing more is started on the card)
                print(f"{name}_{rnd + 1} FAILED rc {p.returncode}\n{p.stderr[-3000:]}", flush=True)
                return 1
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
            r = json.loads(line)
            res[name].append(dict(flatten(r)))
            f = res[name][-1]
            print(f"{name}_{rnd + 1}   value {f['value']:14.1f}  ms_per_step {f.get('ms_per_step', float('nan')):.4f}  "
                  f"avg_kernel_ms {f.get('roofline/avg_kernel_ms', float('nan')):.4f}", flush=True)
    (na, _), (nb, _) = sides
    keys = sorted(k for k in res[na][0] if k in res[nb][0])
    if not args.all_metrics:
        keys = [k for k in keys if k.split("/")[-1] in ("value", "ms_per_step", "avg_kernel_ms", "wall_s", "median_ms")]
    for k in keys:
        va, vb = (np.array([r[k] for r in res[n] if k in r]) for n in (na, nb))
        if va.size == 0 or vb.size == 0 or np.median(va) == 0:
            continue
        print(f"{k:66s} {na} {np.median(va):.5g} [{va.min():.5g}, {va.max():.5g}] {nb} {np.median(vb):.5g} [{vb.min():.5g}, {vb.max():.5g}]"
              f"  {nb}/{na} {np.median(vb) / np.median(va):.4f}")
    va, vb = (np.array([r["value"] for r in res[n]]) for n in (na, nb))
    apart = va.max() < vb.min() or vb.max() < va.min()
    wider = max(np.ptp(va), np.ptp(vb))
    print(f"# value: ranges {'apart' if apart else 'OVERLAP'}; medians differ by {abs(np.median(vb) - np.median(va)):.4g}, three times the wider "
          f"range is {3 * wider:.4g} -- criterion {'met' if apart and abs(np.median(vb) - np.median(va)) >= 3 * wider else 'MISSED'}")
    da, db = (os.path.join(args.out, "dump_" + n) for n in (na, nb))
    ld = lambda d, f: np.load(os.path.join(d, f + ".npy"))
    sa, sb, ia, ib = ld(da, "status"), ld(db, "status"), ld(da, "iters"), ld(db, "iters")
    ch = np.flatnonzero(ia != ib)
    print(f"dump_{na} vs dump_{nb}: status0 {int((sb == 0).sum())}/{sb.size} ({na} {int((sa == 0).sum())})  iters differ {ch.size}  "
          f"max|du_nom| {np.abs(ld(da, 'u_nom') - ld(db, 'u_nom')).max():.2e}  max|dxu_ss| {np.abs(ld(da, 'xu_ss') - ld(db, 'xu_ss')).max():.2e}  "
          f"mean iters {ia.mean():.4f} / {ib.mean():.4f}")
    for i in ch[:64]:
        print(f"  instance {i}: iterations {int(ia[i])} -> {int(ib[i])}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
