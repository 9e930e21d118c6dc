"""Device time of the explicit law next to the solve it replaces (HIP events on the handle's stream: tmpc_last_kernel_ms).

    python scripts/gpu_law.py [--reps 30] [--out profiles/NAME.txt]

Per 4096 cart-pole N = 10 instances (wave kernel) and per 1024 config-5 instances (synthetic nx 12, nu 4, N 30: block kernel), each call
repeated `reps` times after three warm-up calls, through the device-pointer entries; printed: minimum, median, maximum.
  * the plain solve of the batch (the solve kernels' code objects are the parent commit's byte for byte, measured in the same session);
  * tmpc_law_eval_device with every instance a hit: with the right hints, without hints in insertion order, without hints after reorder;
  * tmpc_law_solve_device at miss shares 0, 10 % and 100 % (the regions of the missing share are taken out of the table);
  * on instances that no stored region holds (a pool of other states, those that miss the table): the plain solve, tmpc_law_solve_device,
    and tmpc_law_eval_device with max_tries 1, 4, 16, all -- the time a miss costs."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import common                                                                   # noqa: E402
from LinearMPCOverNetworks import _native                                        # noqa: E402


def timed(h, call, reps):
    ms = []
    for i in range(reps + 3):
        call()
        t = _native.last_kernel_ms(h)
        _native.synchronize(h)
        if i >= 3:
            ms.append(t)
    return np.asarray(ms)


def measure(label, mpc, X, R, pool, reps, lines):
    import torch
    h = mpc._handle
    B = len(X)
    nx, nu, N = h.nx, h.nu, h.N

    def say(name, ms, extra=""):
        lines.append(f"{label:28s} B = {B:5d}  {name:34s} min {ms.min():8.4f}  median {np.median(ms):8.4f}  max {ms.max():8.4f} ms   ({reps} calls){extra}")
        print(lines[-1], flush=True)

    # a batch in which every instance is answered by a region: the solved instances whose signature is admissible, repeated to B
    sol = mpc._solve(X, R, want_traj=False)
    ids, n_new = _native.law_learn(h, X, R, sol)
    good = np.flatnonzero(ids >= 0)
    pick = good[np.arange(B) % len(good)]
    X, R = np.ascontiguousarray(X[pick]), np.ascontiguousarray(R[pick])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x, r = dev(X), dev(R)
    u = torch.empty((B, N, nu), dtype=torch.float64, device="cuda")
    x0 = torch.empty((B, nx), dtype=torch.float64, device="cuda")
    ss = torch.empty((B, nx + nu), dtype=torch.float64, device="cuda")
    st = torch.empty(B, dtype=torch.int32, device="cuda")
    it = torch.empty(B, dtype=torch.int32, device="cuda")
    reg = torch.empty(B, dtype=torch.int32, device="cuda")
    tr = torch.empty(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    outs = (u.data_ptr(), x0.data_ptr(), ss.data_ptr(), None, st.data_ptr(), it.data_ptr(), reg.data_ptr(), tr.data_ptr())
    solve = lambda: _native.solve_batch_device(h, B, x.data_ptr(), r.data_ptr(), None, u.data_ptr(), x0.data_ptr(), ss.data_ptr(), None, st.data_ptr(), it.data_ptr())
    ev = lambda hint=None, mt=0: _native.law_eval_device(h, B, x.data_ptr(), r.data_ptr(), None, hint, mt, *outs)
    sv = lambda: _native.law_solve_device(h, B, x.data_ptr(), r.data_ptr(), None, None, 0, *outs)
    t_solve = timed(h, solve, reps)
    say("plain solve", t_solve, f"   kernel {_native.kernel_name(h)}")
    ev()
    _native.synchronize(h)
    region = reg.cpu().numpy().copy()
    assert np.all(region >= 0), int((region < 0).sum())
    hint = dev(region.astype(np.int32))
    nreg = len(_native.law_stats(h))
    t_hint = timed(h, lambda: ev(hint.data_ptr()), reps)
    say("law eval, all hits, hinted", t_hint, f"   {nreg} regions; ratio to the plain solve {np.median(t_solve) / np.median(t_hint):.1f}; "
        f"outside the spread: {bool(t_hint.max() < t_solve.min())}")
    t = timed(h, ev, reps)
    say("law eval, all hits, no hints", t, f"   mean tries {tr.cpu().numpy().mean():.1f}")
    _native.law_reorder(h)
    t = timed(h, ev, reps)
    say("law eval, no hints, reordered", t, f"   mean tries {tr.cpu().numpy().mean():.1f}")
    # the hops (tmpc_law_set_hops): the hint is the region of the state before -- a closed loop's hint where the region changes every step
    prev = dev(np.roll(region, 1).astype(np.int32))
    t0 = None
    for mh in (0, 4, 16, 64):
        _native.law_set_hops(h, mh)
        _native.law_hop_stats(h, 0, clear=True)
        t = timed(h, lambda: ev(prev.data_ptr()), reps)
        hs = _native.law_hop_stats(h, 0, clear=True)
        tries = float(tr.cpu().numpy().mean())
        if mh == 0:
            t0, tries0 = np.median(t), tries
            say("law eval, hint of the state before, max_hops 0", t, f"   mean tries {tries:.1f}")
        else:
            n = max(1, int(hs[0] + hs[2] + hs[3] + hs[4] + hs[5]))
            say(f"law eval, hint of the state before, max_hops {mh}", t, f"   mean tries {tries:.1f}; chains: hits {hs[0] / n:.1%}, absent {hs[2] / n:.1%}, cap "
                f"{hs[3] / n:.1%}, two-cycle {hs[4] / n:.1%}, parameter row {hs[5] / n:.1%}, tests per chain {hs[1] / n:.2f}; per instance "
                f"{1e3 * (np.median(t) - t0) / B:+.3f} us against max_hops 0 at {tries - tries0:+.2f} tries")
    _native.law_set_hops(h, 0)
    t_s0 = timed(h, sv, reps)
    say("law solve, 0 % misses", t_s0)
    # take out the regions that answer about 10 % of the batch (the least hit first), then all of them
    words = [_native.law_get_region(h, i)["words"] for i in range(nreg)]
    count = np.bincount(region, minlength=nreg)
    by_hits = np.argsort(count, kind="stable")
    drop = by_hits[:int(np.searchsorted(np.cumsum(count[by_hits]), 0.10 * B, side="right")) + 1]
    _native.law_clear(h)
    _native.law_add(h, np.array([w for i, w in enumerate(words) if i not in set(drop.tolist())]))
    t = timed(h, sv, reps)
    share = float((reg.cpu().numpy() < 0).mean())
    say(f"law solve, {share:.0%} misses", t)
    # instances that no stored region holds: the full table again, asked with the states of `pool` that miss it (repeated to B)
    _native.law_clear(h)
    _native.law_add(h, np.array(words))
    Xp, Rp = pool
    probe = _native.law_eval(h, Xp, Rp, want_traj=False)
    away = np.flatnonzero(probe["region"] < 0)
    lines.append(f"{label:28s} {len(away)} of {len(Xp)} pool states are held by none of the {nreg} regions")
    print(lines[-1], flush=True)
    if len(away) == 0:
        return
    pickm = away[np.arange(B) % len(away)]
    xm, rm = dev(Xp[pickm]), dev(Rp[pickm])
    evm = lambda mt=0: _native.law_eval_device(h, B, xm.data_ptr(), rm.data_ptr(), None, None, mt, *outs)
    evm()
    _native.synchronize(h)
    missing = reg.cpu().numpy() < 0
    svm = lambda: _native.law_solve_device(h, B, xm.data_ptr(), rm.data_ptr(), None, None, 0, *outs)
    solvem = lambda: _native.solve_batch_device(h, B, xm.data_ptr(), rm.data_ptr(), None, u.data_ptr(), x0.data_ptr(), ss.data_ptr(), None, st.data_ptr(), it.data_ptr())
    t_pm = timed(h, solvem, reps)
    say("plain solve, pool states", t_pm)
    t_sm = timed(h, svm, reps)
    say(f"law solve, {missing.mean():.0%} misses (pool)", t_sm, f"   law solve - plain solve = {np.median(t_sm) - np.median(t_pm):.4f} ms")
    for mt in (1, 4, 16, 0):
        t = timed(h, lambda: evm(mt), reps)
        say(f"law eval, pool, max_tries {mt if mt else 'all'}", t, f"   {missing.mean():.0%} misses, mean tries {tr.cpu().numpy().mean():.1f}; per instance "
            f"{1e3 * np.median(t) / B:.3f} us against {1e3 * np.median(t_pm) / B:.3f} us per solve")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    S = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
    XR = S[np.arange(4096) % len(S)]
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True)
    # (the pool: the golden states shrunk and shifted -- other working sets than the ones they were learnt from)
    measure("cart-pole N = 10 (nv 11)", mpc, XR[:, :4], XR[:, 4:], (np.ascontiguousarray(-0.37 * S[:, :4] + 0.011), np.ascontiguousarray(S[:, 4:])), args.reps, lines)
    mpc._close()
    mpc, _ = common.make_mpc("synthetic", 30, True, create=True)
    rng = np.random.default_rng(1)
    box = np.asarray(mpc._Xc.b[:12], dtype=np.float64)         # interior states and position references (tests/shape_cases.tracking_states)
    X = rng.uniform(-0.6, 0.6, (1024, 12)) * box
    R = np.c_[rng.uniform(-0.8, 0.8, 1024) * box[0], np.zeros((1024, 11))]
    Xp = rng.uniform(-0.97, 0.97, (2048, 12)) * box             # (the pool: states and references out to the constraints)
    Rp = np.c_[rng.uniform(-0.97, 0.97, 2048) * box[0], np.zeros((2048, 11))]
    measure("config 5 (nx 12 nu 4 N 30)", mpc, X, R, (Xp, Rp), args.reps, lines)
    mpc._close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
