"""The policy behind the launch lanes and the elastic grid (csrc/tmpc_hazard.hpp, through the tmpc_debug_* exports of include/tmpc.h): the
core size of an elastic launch, which launches are elastic, the lane of every call of a script and the followers words it leaves, the
decision of a surplus workgroup, and the busy-time arithmetic of tmpc_kernel_ms_total on several lanes.  Host-only handles, made-up
addresses that are never dereferenced.  CPU only."""
import numpy as np
import pytest

import common

NX, NU, N, B = 4, 1, 10, 8
ARGS = ("x_k", "ref", "variant", "u_nom", "x_nom0", "xu_ss", "x_nom", "status", "iters")


def call(base):
    """every argument in a block of its own, 64 KiB apart, from `base` on"""
    return {k: base + 0x10000 * i for i, k in enumerate(ARGS)}


@pytest.fixture(scope="module")
def host_handles(hip_lib):
    wave, _ = common.make_mpc("cartpole", N, True, create=True, device=-1)
    block, _ = common.make_mpc("cartpole", N, True, create=True, device=-1)
    block.set_kernel_path("block")
    yield wave._handle, block._handle         # (the controllers own their handles: both live as long as the module's tests)
    del wave, block


@pytest.mark.parametrize("n_cu,want", [(1, (1, 1, 1)), (3, (3, 2, 1)), (256, (256, 128, 86)), (304, (304, 152, 102))])
def test_core_size(hip_lib, host_handles, n_cu, want):
    """ceil(n_cu / (lanes - 1)): every lane but one may hold a younger call; two lanes keep the whole grid"""
    h = host_handles[0]
    got = tuple(hip_lib.elastic_grid(h, n_cu, lanes, 8, 1 << 20)[0] for lanes in (2, 3, 4))
    assert got == want
    for lanes, core in zip((2, 3, 4), got):
        assert core * (lanes - 1) >= n_cu > (core - 1) * (lanes - 1)
    assert hip_lib.elastic_grid(h, n_cu, 1, 8, 1 << 20) == (n_cu, False)


def test_eligibility(hip_lib, host_handles):
    wave, block = host_handles
    for n_cu, wpb in ((256, 8), (256, 4), (304, 8), (3, 2)):
        thr = 2 * n_cu * wpb
        for lanes in (3, 4):
            assert hip_lib.elastic_grid(wave, n_cu, lanes, wpb, thr - 1)[1] is False
            assert hip_lib.elastic_grid(wave, n_cu, lanes, wpb, thr)[1] is True
            assert hip_lib.elastic_grid(wave, n_cu, lanes, wpb, 16 * thr)[1] is True
        # two lanes (and one): the core is the whole grid, nothing is elastic -- the two-lane handle's launches as they were
        assert hip_lib.elastic_grid(wave, n_cu, 2, wpb, 16 * thr) == (n_cu, False)
        # a handle with a variant on the block kernel keeps two lanes
        for lanes in (2, 3, 4):
            assert hip_lib.elastic_grid(block, n_cu, lanes, wpb, 16 * thr) == (n_cu, False)
    # one CU: no surplus workgroup to be elastic with
    assert hip_lib.elastic_grid(wave, 1, 4, 8, 1 << 20) == (1, False)
    assert hip_lib.get_call_lanes(block) <= 2 <= hip_lib.MAX_LANES


def test_surplus_decision(hip_lib):
    for lanes in (2, 3, 4):
        for f in range(0, 8):
            assert hip_lib.surplus_yields(f, lanes) == (f >= lanes - 1)
    assert not hip_lib.surplus_yields(100, 1)


def test_independent_calls_rotate_and_count_their_followers(hip_lib):
    calls = [(B, call(0x1000000 * (k + 1))) for k in range(10)]
    for lanes in (1, 2, 3, 4):
        plan = hip_lib.plan_lanes(NX, NU, N, lanes, calls)
        assert [p[0] for p in plan] == [k % lanes for k in range(10)]
        assert all(p[1] == 0 for p in plan)
        # nothing finishes: every later call runs beside call k unless it shares its lane
        want = [sum(1 for j in range(k + 1, 10) if j % lanes != k % lanes) for k in range(10)]
        assert [p[2] for p in plan] == want
    # every call but the first changes lane, so the two entries of tmpc_debug_lane_counters (the parity of the lane changes) alternate
    for lanes in (2, 3, 4):
        lane = [p[0] for p in hip_lib.plan_lanes(NX, NU, N, lanes, calls)]
        assert all(a != b for a, b in zip(lane, lane[1:]))


def test_scripted_hazards_on_four_lanes(hip_lib):
    a, b, c, d = (call(0x1000000 * k) for k in (1, 2, 3, 4))
    raw_a = dict(call(0x5000000), x_k=a["x_nom0"])                    # reads what a writes
    waw_bc = dict(call(0x6000000), u_nom=b["u_nom"], status=c["status"])      # writes what b and c write
    war_d = dict(call(0x7000000), x_nom0=d["x_k"])                    # writes what d reads
    e = call(0x8000000)
    script = [a, b, c, d, raw_a, waw_bc, war_d, e]
    plan = hip_lib.plan_lanes(NX, NU, N, 4, [(B, s) for s in script])
    lane, waited, fol = ([p[i] for p in plan] for i in range(3))
    assert lane[:4] == [0, 1, 2, 3] and waited[:4] == [0, 0, 0, 0]
    # raw_a follows d (lane 3): the rotation reaches lane 0 first, where the call it depends on is -- behind it, no wait
    assert lane[4] == 0 and waited[4] == 0
    # waw_bc follows a call on lane 0: it goes behind b on lane 1 and that lane waits for lane 2
    assert lane[5] == 1 and waited[5] == 1 << 2
    # war_d follows a call on lane 1: lanes 2, then 3, where d is
    assert lane[6] == 3 and waited[6] == 0
    # e is independent: the lane after 3
    assert lane[7] == 0 and waited[7] == 0
    # followers: a call raises the words of the unfinished calls of the OTHER lanes when its lane waits for none; waw_bc raises none
    beside = {0: [1, 2, 3, 4, 6, 7], 1: [2, 3, 4, 6, 7], 2: [3, 4, 6, 7], 3: [4, 7], 4: [6], 5: [6, 7], 6: [7], 7: []}
    for k, later in beside.items():
        assert fol[k] == sum(1 for j in later if lane[j] != lane[k]), (k, fol[k])
    # the same script on two lanes is the two-lane handle's rule: a conflict with the lane of the call before keeps the call there
    plan2 = hip_lib.plan_lanes(NX, NU, N, 2, [(B, s) for s in script])
    # (waw_bc follows raw_a on lane 0, which holds c: it stays there and lane 0 waits for lane 1, where b is)
    assert [p[0] for p in plan2] == [0, 1, 0, 1, 0, 0, 1, 0]
    assert [p[1] for p in plan2] == [0, 0, 0, 0, 0, 1 << 1, 0, 0]
    # a dependent chain never leaves its lane and raises no followers word
    chain, x = [], 0x9000000
    for k in range(6):
        s = dict(call(0xa000000 + 0x1000000 * k), x_k=x)
        chain.append((B, s))
        x = s["x_nom0"]
    assert hip_lib.plan_lanes(NX, NU, N, 4, chain) == [(0, 0, 0)] * 6


def exact_union(start, end):
    order = np.argsort(start, kind="stable")
    total, hi = 0.0, -np.inf
    for i in order:
        total += max(0.0, end[i] - max(start[i], hi))
        hi = max(hi, end[i])
    return total


@pytest.mark.parametrize("lanes", [1, 2, 3, 4])
def test_busy_union_on_overlapping_lanes(hip_lib, lanes):
    """calls in rotation over the lanes, each lane's calls back to back with a random gap now and then, given in the order they start:
    the sum of the extensions is the measure of the union of the intervals"""
    rng = np.random.default_rng(lanes)
    n = 60
    free = np.zeros(lanes)
    start, end, lane = [], [], []
    t = 0.0
    for k in range(n):
        l = k % lanes
        t = max(t, free[l]) + (rng.uniform(0.0, 0.4) if rng.random() < 0.3 else 0.0)
        if k == 30:
            t = max(free.max(), t) + 1.0          # the handle idle for a while
        dur = rng.uniform(0.05, 1.0)
        start.append(t); end.append(t + dur); lane.append(l)
        free[l] = t + dur
    start, end = np.array(start), np.array(end)
    assert np.all(np.diff(start) >= 0)
    got = hip_lib.busy_union(lane, start, end)
    assert got == pytest.approx(exact_union(start, end), rel=1e-12)
    if lanes == 1:
        assert got == pytest.approx(float(np.sum(end - start)), rel=1e-12)
    else:
        assert got < np.sum(end - start)


def test_busy_union_hand_made_cases(hip_lib):
    # three lanes overlap, the third call ends inside the second: 0 .. 5
    assert hip_lib.busy_union([0, 1, 2], [0.0, 1.0, 2.0], [3.0, 5.0, 4.0]) == pytest.approx(5.0)
    # four lanes, every call starts before the one before it ends and ends after it: 0 .. 7
    assert hip_lib.busy_union([0, 1, 2, 3], [0.0, 1.0, 2.0, 3.0], [4.0, 5.0, 6.0, 7.0]) == pytest.approx(7.0)
    # ... and the next call of lane 0 starts after a gap: its own time in full
    assert hip_lib.busy_union([0, 1, 2, 3, 0], [0.0, 1.0, 2.0, 3.0, 9.0], [4.0, 5.0, 6.0, 7.0, 10.5]) == pytest.approx(8.5)
    # a call of another lane that starts after the busy period so far adds its own time, not the gap
    assert hip_lib.busy_union([0, 1], [0.0, 4.0], [1.0, 6.0]) == pytest.approx(3.0)
    assert hip_lib.busy_union([], [], []) == 0.0
