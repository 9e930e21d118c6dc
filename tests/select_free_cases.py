"""Inputs of the select-free factor / back substitution tests (tests/test_select_free_host.py on the host execution model,
tests/test_select_free_gpu.py on the device) in the layout of wavecheck_lanes and tests/wavesim/selectfree_main.cpp:
rows[P][64][n] is the matrix row every lane holds, b1 / b2[P][64] its right-hand-side entries.  Every 16-lane row of the wave gets a
matrix of its own; the lanes >= n of a row hold a copy of its row 0 with zero right-hand sides, as the kernels leave them."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 64
KEYS = ("frows", "dinv", "x", "x2", "ok")


def spd(n, cond, rng):
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    a = (q * np.logspace(0.0, -np.log10(cond), n)) @ q.T
    return 0.5 * (a + a.T)


def lay(n, mats, b1, b2):
    """mats[P][4][n][n], b1 / b2[P][4][n] -> rows[P][64][n], b1 / b2[P][64]"""
    P = mats.shape[0]
    rows, o1, o2 = np.empty((P, L, n)), np.zeros((P, L)), np.zeros((P, L))
    for r in range(4):
        for l in range(16):
            rows[:, 16 * r + l] = mats[:, r, l if l < n else 0]
            if l < n:
                o1[:, 16 * r + l], o2[:, 16 * r + l] = b1[:, r, l], b2[:, r, l]
    return rows, o1, o2


def random_problems(n, P=6, seed=0):
    """P waves of four SPD matrices each, condition numbers 1 ... 1e8, two right-hand sides"""
    rng = np.random.default_rng(1000 * n + seed)
    conds = [1.0, 1e2, 1e4, 1e8]
    mats = np.stack([np.stack([spd(n, conds[(p + r) % 4], rng) for r in range(4)]) for p in range(P)])
    return lay(n, mats, rng.standard_normal((P, 4, n)), rng.standard_normal((P, 4, n)))


def bad_pivot_problems(n, seed=1):
    """a negative pivot at the first, a middle and the last elimination step (one wave each; 16-lane row 0 decides the flag, the
    other rows keep good matrices): A = L diag(d) L' with d_k < 0"""
    rng = np.random.default_rng(2000 * n + seed)
    steps = sorted({0, n // 2, n - 1})
    mats = np.empty((len(steps), 4, n, n))
    for p, k in enumerate(steps):
        for r in range(4):
            lo = np.tril(rng.standard_normal((n, n)) * 0.3, -1) + np.eye(n)
            d = rng.uniform(0.5, 2.0, n)
            if r == 0:
                d[k] = -d[k]
            a = (lo * d) @ lo.T
            mats[p, r] = 0.5 * (a + a.T)
    return steps, lay(n, mats, rng.standard_normal((len(steps), 4, n)), rng.standard_normal((len(steps), 4, n)))


def dyadic_problems(n, P=8, seed=3, negative=None):
    """Matrices whose elimination is EXACT in float64 with pivots that are powers of two: A = L diag(d) L', L unit lower triangular
    with entries in {-4 ... 4} / 8, d_k = 2^e, e in -3 ... 3 (every Schur complement entry is a short sum of such products).  The
    reciprocal of a power of two is exact on the device (v_rcp_f64) and in the host model (a 14-bit seed) alike, and the Newton steps
    leave it alone, so the two sides -- whose reciprocals of a general pivot may differ in the last place -- see the same 1 / d_k;
    the right-hand sides are arbitrary doubles, so the substitutions round at every step.  negative = k: d_k = -2^e in 16-lane row 0."""
    rng = np.random.default_rng(4000 * n + seed)
    mats = np.empty((P, 4, n, n))
    for p in range(P):
        for r in range(4):
            lo = np.tril(rng.integers(-4, 5, (n, n)) / 8.0, -1) + np.eye(n)
            d = 2.0 ** rng.integers(-3, 4, n)
            if negative is not None and r == 0:
                d[negative[p]] = -d[negative[p]]
            mats[p, r] = (lo * d) @ lo.T
            assert np.array_equal(mats[p, r], mats[p, r].T)
    return lay(n, mats, rng.standard_normal((P, 4, n)), rng.standard_normal((P, 4, n)))


def infinity_problems(n, seed=2):
    """an infinity in one lane of the carried right-hand side (waves 0, 1) and of the second one (waves 2, 3): at the step that
    broadcasts that lane, the lanes the triangular pattern excludes multiply it by their zero multiplier -- a NaN with the select
    forms, and so it must be with the masked ones; a form that skipped those lanes would leave them finite"""
    rows, b1, b2 = random_problems(n, P=4, seed=seed)
    for w, l in enumerate([n // 2, n - 1]):
        b1[w, 16 * w + l] = np.inf
        b2[2 + w, 16 * (w + 1) + l] = -np.inf if w else np.inf
    return rows, b1, b2


def run(exe, n, rows, b1, b2, work_dir, tag, env=None):
    """-> (exit code, stderr, {"select": outputs, "masked": outputs}); outputs as Harness.lanes of tests/test_wave_primitives_gpu.py"""
    P = rows.shape[0]
    inp, outp = os.path.join(work_dir, f"in_{tag}.bin"), os.path.join(work_dir, f"out_{tag}.bin")
    np.concatenate([np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (rows, b1, b2)]).tofile(inp)
    res = subprocess.run([exe, str(n), inp, outp], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    if res.returncode not in (0, 1):
        return res.returncode, res.stderr, None
    raw = np.fromfile(outp, dtype=np.float64)
    per = P * L * (n + 4)
    assert raw.size == 2 * per, (raw.size, per)
    forms = {}
    for h, name in enumerate(("select", "masked")):
        part, off, o = raw[h * per:(h + 1) * per], 0, {}
        for key, cnt in (("frows", n), ("dinv", 1), ("x", 1), ("x2", 1), ("ok", 1)):
            o[key] = part[off:off + P * L * cnt].reshape((P, L, n) if key == "frows" else (P, L))
            off += P * L * cnt
        forms[name] = o
    return res.returncode, res.stderr, forms


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
