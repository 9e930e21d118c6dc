"""TEST INFRASTRUCTURE: drives tests/wavesim/seriessim_* (the reduction kernel of csrc/tmpc_series.hip on the host execution model;
the file format is described in seriessim_main.cpp), and the edge-shape record both the host-model test and the GPU test reduce."""

import numpy as np

from hostsim import run_files

INT_TABLES = ("n_alive", "n_nan", "lost_up", "lost_down", "adopted", "tube", "not_optimal", "overrun", "age_max", "iters_max")
LONG_TABLES = ("age_sum", "iters_sum")
REAL_TABLES = ("e_sum", "e_max")
EXACT = INT_TABLES + LONG_TABLES + ("e_max", "e_q")            # equal by bytes between the kernel and the numpy twin
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2049)             # the groups of the edge record: around the wave, the workgroup and eight strides of it
QUANTILES = (0.0, 1.0, 0.5, 0.95, 0.25)                        # 0.25 (n - 1) is an integer for n = 1, 65, 257, 2049; 0.5 (n - 1) for the odd n


def run_stats(binary, e, word, group, q, G, env=None):
    """One launch of the reduction on e, word (T, B) with group (B,) (None: everybody in group 0) -> the tables of montecarlo.series_stats, stderr."""
    e, word = np.asarray(e, dtype=np.float64), np.asarray(word, dtype=np.uint32)
    T, B = word.shape
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    g = np.zeros(B, np.int32) if group is None else np.asarray(group, dtype=np.int32)
    raw, err = run_files(binary, "stats", [np.array([B, T, G, q.size], dtype=np.int64), q, g, e, word], env)
    n, off, out = T * G, 0, {}
    for names, dt in ((INT_TABLES, np.int32), (LONG_TABLES, np.int64), (REAL_TABLES, np.float64)):
        for k in names:
            out[k] = np.frombuffer(raw, dtype=dt, count=n, offset=off).reshape(T, G).copy()
            off += n * np.dtype(dt).itemsize
    out["e_q"] = np.frombuffer(raw, dtype=np.float64, count=n * q.size, offset=off).reshape(T, G, q.size).copy()
    assert off + 8 * n * q.size == len(raw), (off, len(raw))
    out["stderr"] = err
    return out


def edge_record(sizes=SIZES, seed=7):
    """e, word (3, B), group (B,), G: interleaved groups of the given sizes (ids in their order), seven trajectories in no group (-1) and a
    last group of twenty whose words are all 0.  Row 0: every grouped entry alive, all values equal.  Row 1: nine in ten alive, values
    1 + k 2^-52, k = 0 .. 3, of either sign: neighbours in the last bit, many ties.  Row 2: magnitudes 1e-300 .. 1e300 of either sign, and
    among the alive a few +inf and a few NaN; NaN also where nobody is alive.  The words' other bits, iterations and ages are random, the
    saturated 4095 among them.  No -0.0."""
    rng = np.random.default_rng(seed)
    G = len(sizes) + 1
    group = np.concatenate([np.full(n, g, np.int32) for g, n in enumerate(sizes)] + [np.full(7, -1, np.int32), np.full(20, G - 1, np.int32)])
    group = group[rng.permutation(group.size)]
    B = group.size
    word = rng.integers(0, 128, (3, B), dtype=np.uint32) & np.uint32(0x7e)
    word |= rng.choice(np.array([0, 1, 17, 4094, 4095], np.uint32), (3, B)) << np.uint32(8)
    word |= rng.choice(np.array([0, 2, 9, 4095], np.uint32), (3, B)) << np.uint32(20)
    alive = np.ones((3, B), bool)
    alive[1:] = rng.uniform(size=(2, B)) < 0.9
    word |= alive.astype(np.uint32)
    word[:, group == G - 1] = 0
    e = np.empty((3, B))
    e[0] = 0.75
    e[1] = (1.0 + rng.integers(0, 4, B) * 2.0 ** -52) * rng.choice([-1.0, 1.0], B)
    e[2] = 10.0 ** rng.uniform(-300, 300, B) * rng.choice([-1.0, 1.0], B)
    e[2, rng.choice(B, 40, replace=False)] = np.inf
    e[2, rng.choice(B, 40, replace=False)] = np.nan
    e[2, ~alive[2]] = np.where(rng.uniform(size=np.count_nonzero(~alive[2])) < 0.3, np.nan, e[2, ~alive[2]])
    return e, word, group, G


def e_sum_bound(e, word, group, G):
    """(T, G): 2 n 2^-52 sum |e| over the finite values that take part -- what two summations of the same n numbers in different orders can
    differ by (each is within (n - 1) u sum |e| of the exact sum, u = 2^-53, to first order; the factor 2 n 2^-52 leaves the higher orders
    room).  inf where a value that takes part is infinite: the sums are then compared as they are."""
    T, B = word.shape
    out = np.zeros((T, G))
    for g in range(G):
        for t in range(T):
            v = e[t, (group == g) & ((word[t] & 1) == 1)]
            v = v[~np.isnan(v)]
            out[t, g] = np.inf if np.isinf(v).any() else 2.0 * v.size * 2.0 ** -52 * np.abs(v).sum()
    return out
