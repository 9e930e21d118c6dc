"""The hops of the explicit law's search, without a GPU (include/tmpc.h: tmpc_law_set_hops; csrc/tmpc_law_wave.hpp: law_find): the keys and
the hash against restatements, the numpy twin (explicit_law.locate with max_hops) against the closed form of the chain on the clipped
family (tests/law_hop_cases.py), the golden cart-pole states on host-only handles, the refusals of the new C entry points, and the
kernels' source -- law_kernel and closed_loop_law -- on the host execution model under the sanitizers.  The kernels themselves run in
tests/test_law_hops_gpu.py.

Bounds.  Region, tries and the six counters are integers and compared exactly.  y of the clipped family: 1e-11 max|y| against the closed
form (tests/test_explicit_law.py's bound for the kernel's source).  Golden states: TOL_U0 = 1e-8 of tests/certificates.py against the
oracle's solutions."""
import os
import sys

import numpy as np
import pytest

import common
import law_cases as lc
import law_hop_cases as hc
from LinearMPCOverNetworks import explicit_law as E
from LinearMPCOverNetworks import montecarlo
from LinearMPCOverNetworks import sensitivity as S
from oracle.oracle import Oracle
from test_law_loop import _oracle_packets, scenario, sim_tables  # noqa: F401  (sim_tables: the fixture with the "three" table)

ROOT = os.path.dirname(common.PKG)
STATES = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
KEYS = ("u_nom", "x_nom0", "xu_ss", "status")
TOL_U0 = 1e-8                             # tests/certificates.py
E_INVALID, E_UNSUPPORTED, E_DEVICE = -1, -2, -3
HITS, TESTS, ABSENT, CAP, CYCLE, PAR = range(6)


# ------------------------------------------------------------------ keys and the hash
def _z_bitwise(i):
    """splitmix64 of i + 1 (include/tmpc.h), restated on numpy's wrapping uint64."""
    with np.errstate(over="ignore"):
        x = np.uint64(i + 1) * np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return int(x)


def test_signature_key_bit_by_bit():
    assert E.signature_key([]) == 0
    assert _z_bitwise(0) == 0xE220A8397B1DCDAF          # splitmix64's first output from the state 0, as published with the generator
    rng = np.random.default_rng(5)
    for nc in (1, 31, 32, 33, 200, 2049):
        for _ in range(6):
            rows = rng.choice(nc, size=rng.integers(0, min(nc, 40) + 1), replace=False)
            want = 0
            for w, word in enumerate(E.words_of(rows, nc)):
                for bit in range(32):
                    if (int(word) >> bit) & 1:
                        want ^= _z_bitwise(32 * w + bit)
            assert E.signature_key(rows) == want
            for i in rng.choice(nc, size=min(nc, 3), replace=False):       # the neighbour across row i, whichever side i is on
                assert E.signature_key(set(int(r) for r in rows) ^ {int(i)}) == want ^ _z_bitwise(int(i))


def test_hash_twin_layout():
    keys = np.array([5, 5 + 64, 5, E.NO_KEY, 6, 5 + 128], dtype=np.uint64)
    slot = E.hash_slots(keys)
    assert len(slot) == 64 and slot[5] == 0 and slot[6] == 1 and slot[7] == 4 and slot[8] == 5 and (slot >= 0).sum() == 4
    assert [E.hash_find(keys, slot, int(k)) for k in keys[:3]] == [0, 1, 0] and E.hash_find(keys, slot, E.NO_KEY) == -1
    assert E.hash_find(keys, slot, 9) == -1 and E.hash_find(keys, slot, 5 + 192) == -1
    assert len(E.hash_slots(np.arange(33, dtype=np.uint64))) == 128 and len(E.hash_slots(np.arange(32, dtype=np.uint64))) == 64


def test_the_library_hash_on_a_host_only_handle(hip_lib):
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True, device=-1)
    try:
        h = mpc._handle
        nc = hip_lib.get_dims(h, 0)[1]
        rng = np.random.default_rng(11)
        sets = [[]] + [sorted(rng.choice(nc, size=rng.integers(1, 4), replace=False).tolist()) for _ in range(150)]
        assert hip_lib.law_find_key(h, 0) == -1                         # nothing stored yet
        ids = hip_lib.law_add(h, np.array([E.words_of(s, nc) for s in sets]))
        stored = {}
        for s, i in zip(sets, ids):
            if i >= 0:
                stored.setdefault(E.signature_key(s), int(i))
        assert len(stored) > 64                                          # (more than one probe sequence, the table beyond its least size)
        for k, i in stored.items():
            assert hip_lib.law_find_key(h, k) == i
        keys = np.zeros(int(ids.max()) + 1, np.uint64)
        for k, i in stored.items():
            keys[i] = k
        slot = E.hash_slots(keys)
        for _ in range(300):                                             # absent sets: a neighbour of a stored one, and keys at random
            s = sets[rng.integers(len(sets))]
            k = E.signature_key(set(s) ^ {int(rng.integers(nc))})
            assert hip_lib.law_find_key(h, k) == stored.get(k, -1) == E.hash_find(keys, slot, k)
            k = int(rng.integers(0, 1 << 63)) * 2 + 1
            assert hip_lib.law_find_key(h, k) == stored.get(k, -1)
        hip_lib.law_reorder(h)                                           # leaves the hash alone
        assert all(hip_lib.law_find_key(h, k) == i for k, i in stored.items())
        hip_lib.law_clear(h)
        assert all(hip_lib.law_find_key(h, k) == -1 for k in stored)
    finally:
        mpc._close()


# ------------------------------------------------------------------ the twin on the clipped family
def _lattice_case(nv):
    c = lc.clipped_case(300 + nv, nv, 2 * nv + 3, 4, 10)
    sets = hc.lattice(c)
    assert len(sets) == 3 ** nv
    table = [E.region_law(c["model"], s) for s in sets]
    assert all(t is not None for t in table)
    return c, sets, table


@pytest.mark.parametrize("nv", [3, 4])
def test_twin_chain_length_is_the_closed_form(nv):
    c, sets, table = _lattice_case(nv)
    R, B = len(sets), c["B"]
    want = np.array([sets.index(s) for s in c["sets"]])
    seen = set()
    for start in range(R):
        st = np.zeros(6, np.int64)
        region, tries, y = E.locate(table, c["P"], hint=np.full(B, start), max_hops=200, nc=c["nc"], stats=st)
        d = np.array([hc.dist(c, sets[start], b) for b in range(B)])
        assert np.array_equal(region, want) and np.array_equal(tries, 1 + d), (nv, start)
        assert np.max(np.abs(y - c["Z"])) <= 1e-12
        assert st.tolist() == [B, int(tries.sum()), 0, 0, 0, 0]
        for b in range(B):
            assert len(hc.path(c, sets[start], b)) == 1 + d[b]
        seen.update(d.tolist())
    assert {0, 1, 2, nv} <= seen


def _walk_tests(order, start, target):
    """Candidates the walk tests until it reaches `target` (its test included): the order without the chain's start."""
    n = 0
    for r in order:
        if r == start:
            continue
        n += 1
        if r == target:
            return n
    return n


@pytest.mark.parametrize("nv", [3, 4])
def test_twin_with_the_path_removed(nv):
    c, sets, table = _lattice_case(nv)
    rng = np.random.default_rng(nv)
    done = 0
    for b in range(c["B"]):
        for start in rng.choice(len(sets), size=8, replace=False):
            p = hc.path(c, sets[start], b)
            if len(p) < 3:
                continue
            cut = int(rng.integers(1, len(p) - 1))                      # an intermediate set: neither the start nor the target
            keep = [i for i, s in enumerate(sets) if s != p[cut]]
            sub = [table[i] for i in keep]
            s_id, t_id = keep.index(start), keep.index(sets.index(c["sets"][b]))
            order = rng.permutation(len(sub))
            st = np.zeros(6, np.int64)
            region, tries, _ = E.locate(sub, c["P"][b:b + 1], hint=[s_id], order=order, max_hops=200, nc=c["nc"], stats=st)
            today, _, _ = E.locate(sub, c["P"][b:b + 1], hint=[s_id], order=order)
            assert region[0] == t_id == today[0]
            assert tries[0] == cut + _walk_tests(order, s_id, t_id), (nv, b, start, cut)
            assert st.tolist() == [0, cut, 1, 0, 0, 0]
            done += 1
    assert done >= 20


@pytest.mark.parametrize("nv", [3, 4])
def test_twin_max_hops_and_max_tries_inside_the_chain(nv):
    c, sets, table = _lattice_case(nv)
    R, B = len(sets), c["B"]
    want = np.array([sets.index(s) for s in c["sets"]])
    order = np.random.default_rng(9).permutation(R)
    for start in (0, R // 2, R - 1):
        d = np.array([hc.dist(c, sets[start], b) for b in range(B)])
        for mh in (1, 2):
            st = np.zeros(6, np.int64)
            region, tries, _ = E.locate(table, c["P"], hint=np.full(B, start), order=order, max_hops=mh, nc=c["nc"], stats=st)
            exp = np.array([1 + d[b] if d[b] <= mh else mh + 1 + _walk_tests(order, start, want[b]) for b in range(B)])
            assert np.array_equal(region, want) and np.array_equal(tries, exp), (nv, start, mh)
            assert st.tolist() == [int((d <= mh).sum()), int(np.minimum(d, mh).sum() + B), 0, int((d > mh).sum()), 0, 0]
        for mt in (1, 2, 3):
            st = np.zeros(6, np.int64)
            region, tries, _ = E.locate(table, c["P"], hint=np.full(B, start), order=order, max_tries=mt, max_hops=200, nc=c["nc"], stats=st)
            assert np.array_equal(region, np.where(d < mt, want, -1)) and np.array_equal(tries, np.minimum(1 + d, mt)), (nv, start, mt)
            assert st.tolist() == [int((d < mt).sum()), int(tries.sum()), 0, 0, 0, 0]     # (max_tries counts in none of the "ended by")


def test_twin_unhinted_start_is_the_first_of_the_order():
    c, sets, table = _lattice_case(3)
    R, B = len(sets), c["B"]
    want = np.array([sets.index(s) for s in c["sets"]])
    order = np.random.default_rng(2).permutation(R)
    d = np.array([hc.dist(c, sets[order[0]], b) for b in range(B)])
    for hint in (None, np.full(B, -1), np.full(B, R)):
        region, tries, _ = E.locate(table, c["P"], hint=hint, order=order, max_hops=200, nc=c["nc"])
        assert np.array_equal(region, want) and np.array_equal(tries, 1 + d)
    region, tries, _ = E.locate(table, c["P"], order=np.zeros(0, np.int64), max_hops=200, nc=c["nc"])       # an empty order: no chain
    assert np.all(region == -1) and np.all(tries == 0)
    region, tries, _ = E.locate(table, c["P"], hint=want, order=np.zeros(0, np.int64), max_hops=200, nc=c["nc"])
    assert np.array_equal(region, want) and np.all(tries == 1)


def _locate_before(table, P, hint=None, order=None, max_tries=0):
    """explicit_law.locate as it was before the hops, restated: the hint, then the order without it."""
    P = np.asarray(P, dtype=np.float64)
    P = P.reshape(-1, P.shape[-1])
    B, R = P.shape[0], len(table)
    order = np.arange(R) if order is None else np.asarray(order, dtype=np.int64).reshape(-1)
    hint = np.full(B, -1) if hint is None else np.broadcast_to(np.asarray(hint, dtype=np.int64).reshape(-1), (B,))
    ny = next((t["Ky"].shape[0] for t in table if t is not None), 0)
    region, tries, y = np.full(B, -1, np.int32), np.zeros(B, np.int32), np.full((B, ny), np.nan)
    for b in range(B):
        p = P[b]
        if not np.isfinite(p).all():
            continue
        hinted = 0 <= hint[b] < R
        for r in ([int(hint[b])] if hinted else []) + [int(r) for r in order if not (hinted and r == hint[b])]:
            if max_tries > 0 and tries[b] >= max_tries:
                break
            tries[b] += 1
            t = table[r]
            if t is not None and np.all(t["S"] @ p + t["s"] >= 0.0):
                region[b], y[b] = r, t["Ky"] @ p + t["ky"]
                break
    return region, tries, y


@pytest.mark.parametrize("nv", [1, 17, 128])
def test_max_hops_zero_is_the_search_as_it_was(nv):
    """The calls of tests/test_explicit_law.py::test_clipped_family_law_and_search."""
    c = lc.clipped_case(100 + nv, nv, 2 * nv + 5, 8, 12)
    own = []
    for s in c["sets"]:
        if s not in own:
            own.append(s)
    sets = own + lc.other_patterns(c, 20, own)
    table = [E.region_law(c["model"], s) for s in sets]
    table.append(None)
    R, P = len(table), c["P"]
    want = np.array([sets.index(s) for s in c["sets"]])
    bad = P.copy()
    bad[0, 0] = np.inf
    rev = np.arange(R)[::-1]
    for kw in (dict(), dict(hint=want), dict(order=rev), dict(hint=(want + 1) % R), dict(hint=np.full(len(P), R)), dict(max_tries=1), dict(max_tries=2),
               dict(order=rev[:3], hint=want, max_tries=1), dict(hint=np.full(len(P), R - 1), max_tries=3)):
        for pp in (P, bad):
            a, b = E.locate(table, pp, max_hops=0, **kw), _locate_before(table, pp, **kw)
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)), kw
            st = np.zeros(6, np.int64)
            E.locate(table, pp, stats=st, **kw)
            assert not st.any()


# ------------------------------------------------------------------ the golden cart-pole states on host-only handles
@pytest.mark.parametrize("which", ["fixed", "free", "variant1"])
def test_golden_states_with_hops(hip_lib, which):
    """The table of tests/test_explicit_law.py::test_golden_states_on_a_host_only_handle, through the twin.  The hint of state b is the
    region of state b - 1: the hit mask with max_hops = 64 is that without hops, the outputs are the oracle's.  The share of hits the
    chain found is printed, not asserted."""
    X, R = STATES[:, :4], STATES[:, 4:]
    if which == "fixed":
        mpc, _ = common.make_mpc("cartpole", 10, True, create=True, device=-1)
        sol, var, k = dict(np.load(os.path.join(common.GOLDEN, "cartpole_N10_oracle.npz"))), None, 0
    elif which == "free":
        mpc, _ = common.make_mpc("cartpole", 10, False, create=True, device=-1)
        sol, var, k = Oracle(mpc._problem_dict()).solve(X, R), None, 0
    else:
        mpc, _ = common.make_mpc("cartpole", 10, True, extended=True, create=True, device=-1)
        var, k = np.ones(len(X), np.uint8), 1
        sol = Oracle(mpc._problem_dict()).solve(X, R, variant=var)
    try:
        tw = S.handle_sensitivity(mpc, X, R, {kk: sol[kk] for kk in KEYS}, variant=var)
        ok = (tw["flag"] & (S.SKIPPED | S.NOT_KKT)) == 0
        m = E.law_model(mpc._handle, k)
        nc = m["G"].shape[0]
        sets = []
        for a in tw["active"][ok]:
            rows = tuple(S.decode_active(a[:(nc + 31) // 32], nc=nc))
            if rows not in sets:
                sets.append(rows)
        table = [E.region_law(m, s) for s in sets]
        table = [t for t in table if t is not None]
        off, tries0, _ = E.locate(table, STATES)
        hint = np.r_[-1, off[:-1]]
        st = np.zeros(6, np.int64)
        on, tries, y = E.locate(table, STATES, hint=hint, max_hops=64, nc=nc, stats=st)
        assert np.array_equal(on >= 0, off >= 0)
        hit = on >= 0
        want = np.c_[sol["u_nom"].reshape(len(X), -1), sol["x_nom0"], sol["xu_ss"]]
        err = float(np.max(np.abs(y[hit] - want[hit])))
        assert err <= TOL_U0, (which, err)
        _, tries_h, _ = E.locate(table, STATES, hint=hint)
        print(f"{which}: {len(table)} regions, {int(hit.sum())} of {len(X)} located; the chain found {st[HITS]} of them "
              f"({st[HITS] / max(1, hit.sum()):.0%}) in {st[TESTS]} tests; ended absent {st[ABSENT]}, cap {st[CAP]}, cycle {st[CYCLE]}, parameter row {st[PAR]}; "
              f"mean tries {tries[hit].mean():.1f} with hops, {tries_h[hit].mean():.1f} with the hint alone, {tries0[hit].mean():.1f} unhinted; "
              f"largest output difference to the oracle {err:.2e}")
        assert st[HITS] + st[ABSENT] + st[CAP] + st[CYCLE] + st[PAR] <= len(X) and st[TESTS] <= tries.sum()
    finally:
        mpc._close()


# ------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def handles(hip_lib):
    import regulator_problems
    plain, _ = common.make_mpc("cartpole", 10, True, create=True, device=-1)
    reg = regulator_problems.plain_double_integrator(device=-1)
    yield dict(plain=plain._handle, reg=reg._handle)
    plain._close()
    reg._close()


def test_set_hops_stores_the_value_on_a_host_only_handle(hip_lib, handles):
    h = handles["plain"]
    assert hip_lib.law_get_hops(h) == 0
    hip_lib.law_set_hops(h, 7)
    assert hip_lib.law_get_hops(h) == 7
    assert hip_lib.lib().tmpc_law_set_hops(h.ptr, -1) == E_INVALID and h.error() == "tmpc_law_set_hops: max_hops < 0"
    assert hip_lib.law_get_hops(h) == 7                                   # a refused call changes nothing
    hip_lib.law_set_hops(h, 0)
    assert not hip_lib.law_hop_stats(h, 0).any()                          # host-only: zeros
    assert hip_lib.lib().tmpc_law_clear_hop_stats(h.ptr, 0) == 0


def test_null_handles_and_null_arguments_are_refused(hip_lib, handles):
    L, h = hip_lib.lib(), handles["plain"]
    st = np.zeros(6, np.int64)
    i = np.zeros(1, np.int32)
    assert L.tmpc_law_set_hops(None, 1) == E_INVALID and L.tmpc_law_get_hops(None, i.ctypes.data) == E_INVALID
    assert L.tmpc_law_get_hop_stats(None, 0, st.ctypes.data) == E_INVALID and L.tmpc_law_clear_hop_stats(None, 0) == E_INVALID
    assert L.tmpc_law_find_key(None, 0, 0, i.ctypes.data) == E_INVALID
    assert L.tmpc_law_get_hops(h.ptr, None) == E_INVALID and h.error() == "tmpc_law_get_hops: NULL argument"
    assert L.tmpc_law_get_hop_stats(h.ptr, 0, None) == E_INVALID and h.error() == "tmpc_law_get_hop_stats: NULL argument"
    assert L.tmpc_law_find_key(h.ptr, 0, 0, None) == E_INVALID and h.error() == "tmpc_law_find_key: NULL argument"


def test_a_variant_out_of_range_is_refused(hip_lib, handles):
    L, h = hip_lib.lib(), handles["plain"]
    st = np.zeros(6, np.int64)
    i = np.zeros(1, np.int32)
    for rc in (L.tmpc_law_get_hop_stats(h.ptr, 1, st.ctypes.data), L.tmpc_law_clear_hop_stats(h.ptr, -1), L.tmpc_law_find_key(h.ptr, 2, 0, i.ctypes.data)):
        assert rc == E_INVALID and "variant out of range" in h.error()


@pytest.mark.parametrize("name", ["tmpc_law_set_hops", "tmpc_law_get_hops", "tmpc_law_get_hop_stats", "tmpc_law_clear_hop_stats", "tmpc_law_find_key"])
def test_a_regulator_handle_is_refused(hip_lib, handles, name):
    L, h = hip_lib.lib(), handles["reg"]
    buf = np.zeros(6, np.int64)
    rc = {"tmpc_law_set_hops": lambda: L.tmpc_law_set_hops(h.ptr, 1), "tmpc_law_get_hops": lambda: L.tmpc_law_get_hops(h.ptr, buf.ctypes.data),
          "tmpc_law_get_hop_stats": lambda: L.tmpc_law_get_hop_stats(h.ptr, 0, buf.ctypes.data),
          "tmpc_law_clear_hop_stats": lambda: L.tmpc_law_clear_hop_stats(h.ptr, 0), "tmpc_law_find_key": lambda: L.tmpc_law_find_key(h.ptr, 0, 0, buf.ctypes.data)}[name]()
    assert rc == E_UNSUPPORTED and "regulator handle" in h.error(), (name, rc, h.error())


def test_refusals_of_the_handle_free_entry_with_hops(hip_lib):
    c = lc.clipped_case(1, 4, 8, 3, 2)
    m = c["model"]
    args = (m["H"], m["F"], m["G"], m["g0"], m["Ebar"], m["Y"], m["Yp"], np.zeros((2, 1), np.uint32), np.arange(2), c["P"])
    with pytest.raises(ValueError, match=r"tmpc_qp_law_eval_hops: max_hops < 0"):
        hip_lib.qp_law_eval(*args, max_hops=-1, device=-1)
    with pytest.raises(Exception, match=r"tmpc_qp_law_eval_hops: device < 0"):
        hip_lib.qp_law_eval(*args, max_hops=3, device=-1)
    with pytest.raises(Exception, match=r"tmpc_qp_law_eval: device < 0"):
        hip_lib.qp_law_eval(*args, device=-1)
    with pytest.raises(ValueError, match=r"tmpc_qp_law_eval_hops: order\[1\] is not a set"):
        hip_lib.qp_law_eval(*args[:8], np.array([0, 2]), c["P"], max_hops=3, device=-1)


def test_law_setting_accepts_max_hops(hip_lib):
    assert hip_lib._law_setting(dict(max_tries=2, miss_capacity=9, max_hops=5)) == (1, 2, 9) and hip_lib._law_hops(dict(max_hops=5)) == 5
    assert hip_lib._law_hops(dict(max_tries=2)) is None and hip_lib._law_hops(True) is None and hip_lib._law_hops(None) is None
    with pytest.raises(ValueError, match="unknown keys"):
        hip_lib._law_setting(dict(hops=3))


def test_a_loop_puts_the_handles_hops_back(hip_lib, handles):
    """law=dict(max_hops=) holds for the loop it is given to: the handle's own value comes back when the loop's result is assembled, or
    before the next loop's settings where the loop failed."""
    h = handles["plain"]
    hip_lib.law_set_hops(h, 3)
    hip_lib._set_loop_options(h, False, False, None, law=dict(max_hops=16))
    assert hip_lib.law_get_hops(h) == 16
    hip_lib._restore_law_hops(h)
    assert hip_lib.law_get_hops(h) == 3
    hip_lib._restore_law_hops(h)                                          # nothing pending: nothing changes
    assert hip_lib.law_get_hops(h) == 3
    hip_lib._set_loop_options(h, False, False, None, law=dict(max_hops=16))         # a loop that failed before its end ...
    hip_lib._set_loop_options(h, False, False, None, law=True)                      # ... is undone by the next loop's settings
    assert hip_lib.law_get_hops(h) == 3
    hip_lib._set_loop_options(h, False, False, None, law=None)
    hip_lib.law_set_hops(h, 0)


# ------------------------------------------------------------------ the kernels' source on the host execution model
@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    """The host-model programs under the sanitizers (tests/wavesim/hostsim.py: a host without their runtimes skips, a program that does not
    build fails).  Stand-alone programs: nothing is loaded into Python under a sanitizer."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "wavesim"))
    import hostsim
    import law_hop_case
    import law_loop_hop_case
    return law_hop_case, law_loop_hop_case, {**hostsim.binaries_or_skip(tmp_path_factory, "lawhop"), **hostsim.binaries_or_skip(tmp_path_factory, "lawloophop")}


def _clean(out):
    import hostsim
    hostsim.assert_clean(out["stderr"])


@pytest.mark.parametrize("build", ["lawhop_asan", "lawhop_msan"])
@pytest.mark.parametrize("shape", [(1, 2, 1), (17, 65, 8), (128, 2049, 32)])
def test_kernel_source_with_hops_on_the_host_model(binaries, build, shape):
    """csrc/tmpc_law.hip compiled for the CPU under ASan + UBSan and under MSan: the clipped family with B in {1, 65}, the table the paths
    from a common start (tests/law_hop_cases.py: hop_table) and a refused set, hints valid, absent and out of range: region, tries, the
    hit counters and the chains' six counters equal the twin's, y the closed form."""
    import hostsim
    law_hop_case, _, bins = binaries
    nv, nc, npar = shape
    for B in (1, 65):
        c = lc.clipped_case(11 * nv + B, nv, nc, npar, B)
        # (the start: three hops from the first instance's own set, far from most others; the widest shape keeps few whole paths)
        sets, start, full = hc.hop_table(c, c["sets"][0][3:], 12 if nv == 128 else 400, seed=B)
        table = [E.region_law(c["model"], s) for s in sets] + [None]
        assert all(t is not None for t in table[:-1]) and (any(full) or nv == 1)
        R = len(table)
        order = np.random.default_rng(B).permutation(R)
        hint = np.array([(start, -1, R, R - 1)[b % 4] for b in range(B)], np.int32)
        for mh, mt, hn in ((200, 0, hint), (1, 0, hint), (200, 2, hint), (3, 0, None), (0, 0, hint)):
            out = law_hop_case.run(bins[build], table, c["P"], hint=hn, order=order, max_tries=mt, max_hops=mh, nc=nc, env=hostsim.SAN_ENV)
            _clean(out)
            st = np.zeros(6, np.int64)
            region, tries, y = E.locate(table, c["P"], hint=hn, order=order, max_tries=mt, max_hops=mh, nc=nc, stats=st)
            assert np.array_equal(out["region"], region) and np.array_equal(out["tries"], tries), (shape, B, mh, mt)
            assert np.array_equal(out["stats"], st), (shape, B, mh, mt, out["stats"], st)
            hit = region >= 0
            assert np.all(np.isnan(out["y"][~hit]))
            assert np.max(np.abs(out["y"][hit] - c["Z"][hit]), initial=0.0) <= 1e-11 * max(1.0, float(np.abs(c["Z"]).max()))
            assert np.array_equal(out["hits"], np.bincount(region[hit], minlength=R).astype(np.uint64))
            if mh == 200 and mt == 0:
                assert hit.all() and st[HITS] >= sum(full[b] for b in range(B) if hint[b] == start)


def _fabricated(nrow=70, npar=3, ny=2):
    """Raw rows, no QP behind them.  Regions 0 and 1 (working sets {3} and {3, 5}) both fail in row 5 and nowhere below: they send the chain
    to each other.  Region 2 fails in row 68 alone, a parameter-only row with nc = 66.  Region 3 holds every p, region 4 (the set {9}) fails
    in row 9, whose neighbour -- the empty set -- is region 3."""
    def reg(rows, fail):
        s = np.ones(nrow)
        s[list(fail)] = -1.0
        return dict(rows=np.array(sorted(rows), np.int64), S=np.zeros((nrow, npar)), s=s, Ky=np.ones((ny, npar)) * (1 + len(rows)), ky=np.arange(ny, dtype=np.float64))
    return [reg({3}, (5, 40, 69)), reg({3, 5}, (5, 65)), reg({7}, (68,)), reg(set(), ()), reg({9}, (9, 10))]


@pytest.mark.parametrize("build", ["lawhop_asan", "lawhop_msan"])
def test_two_cycle_and_parameter_row_on_the_host_model(binaries, build):
    import hostsim
    law_hop_case, _, bins = binaries
    table = _fabricated()
    for B in (1, 65):
        P = np.random.default_rng(B).standard_normal((B, 3))
        hint = np.array([(0, 2, 1, 4, -1)[b % 5] for b in range(B)], np.int32)
        for order in (np.array([4, 0, 1, 2, 3]), np.array([1, 3])):
            for mh, mt in ((8, 0), (8, 2), (1, 0)):
                out = law_hop_case.run(bins[build], table, P, hint=hint, order=order, max_tries=mt, max_hops=mh, nc=66, env=hostsim.SAN_ENV)
                _clean(out)
                st = np.zeros(6, np.int64)
                region, tries, y = E.locate(table, P, hint=hint, order=order, max_tries=mt, max_hops=mh, nc=66, stats=st)
                assert np.array_equal(out["region"], region) and np.array_equal(out["tries"], tries) and np.array_equal(out["stats"], st), (B, mh, mt)
                assert np.array_equal(np.isnan(out["y"]), np.isnan(y))
                assert np.nanmax(np.abs(out["y"] - y), initial=0.0) <= 1e-11 * np.nanmax(np.abs(y), initial=1.0)       # (np + 1 fused multiply-adds against a product)
                if B == 65 and (mh, mt) == (8, 0):
                    assert st[CYCLE] > 0 and st[PAR] > 0 and st[HITS] > 0
    # the closed form of the first batch: hint 0 -> 0, 1, back to 0: a two-cycle after two tests, then the walk 4, (0 skipped,) 1, 2, 3
    st = np.zeros(6, np.int64)
    region, tries, _ = E.locate(table, np.zeros((1, 3)), hint=[0], order=np.array([4, 0, 1, 2, 3]), max_hops=8, nc=66, stats=st)
    assert region[0] == 3 and tries[0] == 2 + 4 and st.tolist() == [0, 2, 0, 0, 1, 0]
    st = np.zeros(6, np.int64)
    region, tries, _ = E.locate(table, np.zeros((1, 3)), hint=[2], order=np.array([4, 0, 1, 2, 3]), max_hops=8, nc=66, stats=st)
    assert region[0] == 3 and tries[0] == 1 + 4 and st.tolist() == [0, 1, 0, 0, 0, 1]
    st = np.zeros(6, np.int64)
    region, tries, _ = E.locate(table, np.zeros((1, 3)), hint=[4], max_hops=8, nc=66, stats=st)
    assert region[0] == 3 and tries[0] == 2 and st.tolist() == [1, 2, 0, 0, 0, 0]


@pytest.mark.parametrize("build", ["lawloophop_asan", "lawloophop_msan"])
def test_fused_kernel_source_with_hops_on_the_host_model(binaries, sim_tables, build):  # noqa: F811
    """csrc/tmpc_kernels.hip with FUSED = 3 compiled for the CPU under ASan + UBSan and under MSan (bench shape, B in {1, 9}, T = 3), the
    "three" table of tests/test_law_loop.py with max_hops = 4: region, tries, hits, the per-region counters, the six counters and the miss
    count equal the host twin's (montecarlo.LawPackets(max_hops=4) on the same table, the oracle behind it)."""
    import hostsim
    _, law_loop_hop_case, bins = binaries
    mpc, w, orc, shape, tables = sim_tables
    table = tables["three"]
    nc = E.law_model(mpc._handle, 0)["G"].shape[0]
    T, N = 3, 10
    K, Kp = mpc.get_steady_state_controller_gain(), mpc.get_ancillary_controller_gain()
    for B in (1, 9):
        sc = scenario(w, B, T)
        for max_tries in (0, 2):
            twin = montecarlo.LawPackets.from_tables(_oracle_packets(mpc, orc), table, K, N, ncs=nc, max_tries=max_tries, miss_capacity=B * T, max_hops=4)
            host = montecarlo.run_remote_tube_mpc(twin, w["A"], w["B"], K, Kp, N, mpc._Z, sc["p_loss"], sc["ref"], sc["th_u"], sc["ga_u"], sc["w"])
            res = twin.result()
            out = law_loop_hop_case.run(bins[build], mpc._problem_dict(), K, Kp, mpc._Z, sc["p_loss"], sc["ref"], sc["th_u"], sc["ga_u"], sc["w"], table, shape,
                                        max_tries=max_tries, miss_capacity=B * T, warm=(B == 9), env=hostsim.SAN_ENV, max_hops=4, nc=nc)
            _clean(out)
            assert np.array_equal(out["region"], res["law_region"]) and np.array_equal(out["hits"], res["law_hits"]), (B, max_tries)
            assert np.array_equal(out["tries"], res["law_tries"]), (B, max_tries, out["tries"], res["law_tries"])
            assert np.array_equal(out["stats"], res["hop_stats"][0]), (B, max_tries, out["stats"], res["hop_stats"][0])
            assert out["stats"][TESTS] > 0
            want = np.array([twin.region_hits[0].get(r, 0) for r in range(len(table))], np.uint64)
            assert np.array_equal(out["region_hits"], want)
            assert out["n_total"] == res["misses"]["n_total"] and int(out["hits"].sum()) + out["n_total"] == B * T
            np.testing.assert_allclose(out["x_final"], host["x_final"], atol=1e-7, rtol=0)
            assert np.array_equal(out["not_optimal"], host["not_optimal"]) and np.array_equal(out["tube_violations"], host["tube_violations"])
