"""Probe of v_mfma_f64_4x4x4_4b_f64 on the device (lib/libtmpc_mfmablocks.so, tests/wavecheck/mfmablocks.hip): the lane maps of its
three operands read off one-hot operands, the order of its four additions, and its issue time against v_mfma_f64_16x16x4_f64
(s_memtime around 512 instructions of one wave).  Prints what profiles/r15_mfma_blocks_measure.txt records."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "robust-tracking-mpc-over-lossy-networks_amd", "lib", "libtmpc_mfmablocks.so")
L = 64
_dp = C.POINTER(C.c_double)


def _d(a):
    return a.ctypes.data_as(_dp)


def raw(lib, a, b, c):
    a, b, c = (np.ascontiguousarray(x, dtype=np.float64) for x in (a, b, c))
    d = np.empty_like(a)
    rc = lib.mfmablocks_raw(C.c_int(a.shape[0]), _d(a), _d(b), _d(c), _d(d))
    assert rc == 0, rc
    return d


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))          # one rounding


def main():
    lib = C.CDLL(LIB)
    eye = np.eye(L)
    one = np.ones((L, L))
    zero = np.zeros((L, L))
    SA = raw(lib, eye, one, zero) != 0          # [la][lane of D]
    SB = raw(lib, one, eye, zero) != 0
    pair = raw(lib, np.repeat(eye, L, axis=0), np.tile(eye, (L, 1)), np.zeros((L * L, L))).reshape(L, L, L) != 0   # [la][lb][lane of D]
    meets = pair.any(axis=2)
    print("# lane maps: D lanes that a one-hot A lane / B lane reaches; the B lanes an A lane meets (same block, same k)")
    for l in range(L):
        print(f"lane {l:2d}  A -> D {np.flatnonzero(SA[l]).tolist()}  B -> D {np.flatnonzero(SB[l]).tolist()}  A meets B {np.flatnonzero(meets[l]).tolist()}")
    blk, minor, major = (np.arange(L) >> 2) & 3, np.arange(L) & 3, np.arange(L) >> 4
    wantA = (blk[:, None] == blk[None, :]) & (minor[:, None] == major[None, :])      # A lane (k, b, i) -> D lanes (i, b, *)
    wantB = (blk[:, None] == blk[None, :]) & (minor[:, None] == minor[None, :])      # B lane (k, b, j) -> D lanes (*, b, j)
    wantM = (blk[:, None] == blk[None, :]) & (major[:, None] == major[None, :])
    ok = bool((SA == wantA).all() and (SB == wantB).all() and (meets == wantM).all())
    print(f"maps A: lane 16 k + 4 b + i, B: lane 16 k + 4 b + j, C / D: lane 16 i + 4 b + j -- {'CONFIRMED' if ok else 'NOT what the device does'}")

    # the order of the additions: products and C spread over many decades, against candidates evaluated exactly
    rng = np.random.default_rng(3)
    P = 8
    a, b, c = (rng.choice([-1.0, 1.0], (P, L)) * 10.0 ** rng.uniform(-6.0, 6.0, (P, L)) for _ in range(3))
    d = raw(lib, a, b, c)
    cands = {"fma chain k = 0..3 from C": 0, "fma chain k = 3..0 from C": 0, "products rounded, added to C k = 0..3": 0, "exact sum, one rounding": 0}
    for p in range(P):
        for l in range(L):
            i, bq, j = l >> 4, (l >> 2) & 3, l & 3
            A = [a[p, 16 * k + 4 * bq + i] for k in range(4)]
            B = [b[p, 16 * k + 4 * bq + j] for k in range(4)]
            v = c[p, l]
            for k in range(4):
                v = fma(A[k], B[k], v)
            cands["fma chain k = 0..3 from C"] += v == d[p, l]
            v = c[p, l]
            for k in (3, 2, 1, 0):
                v = fma(A[k], B[k], v)
            cands["fma chain k = 3..0 from C"] += v == d[p, l]
            v = c[p, l]
            for k in range(4):
                v = v + A[k] * B[k]
            cands["products rounded, added to C k = 0..3"] += v == d[p, l]
            cands["exact sum, one rounding"] += float(sum(Fraction(A[k]) * Fraction(B[k]) for k in range(4)) + Fraction(c[p, l])) == d[p, l]
    print("# order of the additions: entries (of %d) that a candidate reproduces to the last bit" % (P * L))
    for k, v in cands.items():
        print(f"{k}: {v}")

    n = lib.mfmablocks_time_insts()
    print(f"# issue time: s_memtime ticks around {n} matrix instructions, one wave in one workgroup; 9 launches each, ticks per instruction min / median / max")
    names = ["blocks 4x4x4_4b, 2 alternating accumulators", "tile 16x16x4, 2 alternating accumulators", "blocks 4x4x4_4b, 1 accumulator (dependent chain)",
             "blocks 4x4x4_4b, 4 alternating accumulators", "tile 16x16x4, 1 accumulator (dependent chain)"]
    for kind, name in enumerate(names):
        cyc = (C.c_longlong * 9)()
        rc = lib.mfmablocks_time(C.c_int(kind), C.c_int(9), cyc)
        assert rc == 0, rc
        v = np.array(list(cyc), dtype=np.float64) / n
        print(f"{name}: {v.min():.2f} / {np.median(v):.2f} / {v.max():.2f}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
