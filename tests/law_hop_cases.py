"""The hops of the explicit law on the clipped family of tests/law_cases.py (NOT a test module): the closed form of the chain.

The problem is separable.  With r = -(F p)_i / d_i the unclipped minimiser of coordinate i, the coordinate is in state U (row i, z_i <= 1,
in the working set), L (row nv + i, -z_i <= 1, in it) or F (neither).  At p the rows of the region of a working set behave so:
    row i      in the set: its multiplier d_i (r - 1), which fails where r < 1;   outside: the slack 1 - z_i, which fails in state F where r > 1;
    row nv + i in the set: its multiplier d_i (-r - 1), which fails where r > -1; outside: the slack 1 + z_i, which fails in state F where r < -1;
the padding rows beyond the box never fail.  The family's margins (|r| at least 0.1 away from 1) decide every one of these tests, at the
intermediate regions of a chain as at its ends.  The rule -- flip the lowest failing row -- therefore moves one coordinate by one state per
hop: a chain from the pattern s to the instance's pattern t tests exactly 1 + sum_i dist(s_i, t_i) regions, dist being 0 between equal
states, 1 between F and U or L, 2 between U and L (through F), over the coordinates whose rows exist."""
import numpy as np


def ratios(c: dict):
    m = c["model"]
    return -(c["P"] @ m["F"].T) / np.diag(m["H"])


def failing_rows(c: dict, rows, r):
    """The failing rows, ascending, of the region of the working set `rows` at an instance with the ratios r (nv,)."""
    nv, A, out = c["nv"], set(int(i) for i in rows), []
    for i in range(nv):
        up, lo = i in A, nv + i in A
        if c["has_up"][i] and (r[i] < 1.0 if up else (not lo and r[i] > 1.0)):
            out.append(i)
        if c["has_lo"][i] and (r[i] > -1.0 if lo else (not up and r[i] < -1.0)):
            out.append(nv + i)
    return sorted(out)


def path(c: dict, start, b: int):
    """The working sets a chain from the set `start` visits for instance b, the start first and the instance's own set last: the rule
    applied to the closed form."""
    r = ratios(c)[b]
    cur, out = sorted(int(i) for i in start), []
    for _ in range(4 * c["nv"] + 2):
        out.append(cur)
        bad = failing_rows(c, cur, r)
        if not bad:
            assert cur == sorted(int(i) for i in c["sets"][b]), (cur, c["sets"][b])
            return out
        cur = sorted(set(cur) ^ {bad[0]})
    raise AssertionError("the chain does not end")


def dist(c: dict, start, b: int) -> int:
    """sum_i dist(s_i, t_i) between the pattern of `start` and that of instance b."""
    nv, s, t = c["nv"], set(int(i) for i in start), set(int(i) for i in c["sets"][b])
    state = lambda A, i: 1 if i in A else (-1 if nv + i in A else 0)
    return int(sum(abs(state(s, i) - state(t, i)) for i in range(nv)))


def lattice(c: dict):
    """Every working set of the box rows that exist, one state per coordinate (3^nv of them where every row exists)."""
    nv, out = c["nv"], [[]]
    for i in range(nv):
        ext = [[]] + ([[i]] if c["has_up"][i] else []) + ([[nv + i]] if c["has_lo"][i] else [])
        out = [sorted(a + e) for a in out for e in ext]
    return out


def hop_table(c: dict, start, max_regions: int, decoys: int = 0, seed: int = 0, keep_rest: bool = True):
    """A table for the chains of case c from the common start `start`: the start, then per instance its whole path while the table stays
    within max_regions sets -- afterwards the first hop of the path and the instance's own set only, so that such a chain ends at an
    absent neighbour and the walk answers, or with keep_rest False nothing: such an instance may miss --, then `decoys` other patterns;
    all in a shuffled order of ids.
    -> (sets, id of the start, full: per instance whether its whole path is in the table)."""
    import law_cases as lc
    sets, full = [sorted(int(i) for i in start)], []
    for b in range(c["B"]):
        p = path(c, start, b)
        new = [s for s in p if s not in sets]
        whole = len(sets) + len(new) <= max_regions
        full.append(whole)
        for s in (p if whole else p[:2] + p[-1:] if keep_rest else []):
            if s not in sets:
                sets.append(s)
    # (a truncated path may be completed by the sets of other instances: `full` is then recomputed from the table itself)
    full = [all(s in sets for s in path(c, start, b)) for b in range(c["B"])]
    sets += lc.other_patterns(c, decoys, sets)
    perm = np.random.default_rng(seed).permutation(len(sets))
    sets = [sets[i] for i in perm]
    return sets, sets.index(sorted(int(i) for i in start)), full
