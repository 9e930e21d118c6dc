"""Two launch lanes per device handle (include/tmpc.h: the ordering contract of tmpc_solve_batch_device, tmpc_set_call_overlap):
successive independent device-pointer calls run side by side, dependent ones stay in call order, every other entry point joins the
lanes first.  The reference of every check is the same sequence of calls with tmpc_synchronize between them; outputs must agree BIT FOR
BIT (a solve's arithmetic does not depend on what runs beside it), and the lane counters (tmpc_debug_lane_counters) say where the calls
went -- a timing assertion would be flaky.  Nothing here provokes a fault: a wrong hazard rule shows as a mismatch (an input read
before the call that writes it has run is still the NaN fill)."""
import os
import time

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

S = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
NX, NU, N = 4, 1, 10
B = 4096                 # two rounds of the card's resident waves: a call lasts far longer than the host needs to enqueue the next one
ARGS = ("x_k", "ref", "variant", "u_nom", "x_nom0", "xu_ss", "x_nom", "status", "iters")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def plain(hip_lib):
    mpc, w = common.make_mpc("cartpole", N, True, create=True)
    return mpc, w


@pytest.fixture(scope="module")
def extended(hip_lib):
    mpc, w = common.make_mpc("cartpole", N, True, extended=True, create=True)
    return mpc, w


def states(seed, b=B):
    """b rows of the fixture states in a seeded random order (with repetition)"""
    i = np.random.default_rng(seed).integers(0, len(S), b)
    return np.ascontiguousarray(S[i, :NX]), np.ascontiguousarray(S[i, NX:])


class Buffers:
    """Named device arrays with their initial contents: outputs start as NaN / -1, so that a call that ran too early is seen."""

    def __init__(self, torch):
        self.torch, self.dev, self.t, self.init = torch, torch.device("cuda:0"), {}, {}

    def put(self, name, array):
        self.init[name] = np.ascontiguousarray(array)
        self.t[name] = self.torch.from_numpy(self.init[name]).to(self.dev)
        return name

    def outputs(self, name, b=B, traj=False):
        """the output arrays of one call, named name.u_nom ...; -> {argument: buffer name}"""
        shapes = {"u_nom": (b, N, NU), "x_nom0": (b, NX), "xu_ss": (b, NX + NU), "status": (b,), "iters": (b,)}
        if traj:
            shapes["x_nom"] = (b, N + 1, NX)
        return {k: self.put(f"{name}.{k}", np.full(s, -1, np.int32) if k in ("status", "iters") else np.full(s, np.nan)) for k, s in shapes.items()}

    def reset(self):
        for k, a in self.init.items():
            self.t[k].copy_(self.torch.from_numpy(a))
        self.torch.cuda.synchronize()

    def snapshot(self):
        self.torch.cuda.synchronize()
        return {k: v.cpu().numpy().copy() for k, v in self.t.items()}

    def solve(self, hip, h, call, b=B):
        hip.solve_batch_device(h, b, *[None if call.get(k) is None else self.t[call[k]].data_ptr() for k in ARGS])


def run(hip, h, bufs, calls, fenced, after=None):
    """the calls in order, with tmpc_synchronize after each one (`fenced`) or not; then `after()`; -> (every buffer, after's result,
    lane counters of the sequence)"""
    bufs.reset()
    hip.synchronize(h)
    hip.lane_counters(h, reset=True)
    for c in calls:
        bufs.solve(hip, h, c)
        if fenced:
            hip.synchronize(h)
    extra = after() if after else None
    hip.synchronize(h)
    return bufs.snapshot(), extra, hip.lane_counters(h)


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def independent_calls(bufs, K, with_variant):
    calls = []
    for k in range(K):
        X, R = states(100 + k)
        c = {"x_k": bufs.put(f"c{k}.x", X), "ref": bufs.put(f"c{k}.r", R), **bufs.outputs(f"c{k}", traj=(k % 4 == 0))}
        if with_variant:
            c["variant"] = bufs.put(f"c{k}.g", np.random.default_rng(200 + k).integers(0, 2, B).astype(np.uint8))
        calls.append(c)
    return calls


@pytest.mark.parametrize("which", ["plain", "extended"])
def test_independent_calls_alternate_and_agree_bit_for_bit(hip_lib, torch, plain, extended, which):
    mpc = (plain if which == "plain" else extended)[0]
    h = mpc._handle
    K = 16
    bufs = Buffers(torch)
    calls = independent_calls(bufs, K, with_variant=(which == "extended"))
    hip_lib.set_call_overlap(h, True)
    got, _, ((n0, n1), waits) = run(hip_lib, h, bufs, calls, fenced=False)
    want, _, _ = run(hip_lib, h, bufs, calls, fenced=True)
    same(got, want)
    print(f"{which}: calls per lane ({n0}, {n1}), cross-lane waits {waits}")
    assert n0 + n1 == K and waits == 0
    # the second lane exists from the first call on that finds the call before it unfinished; from then on the calls alternate
    assert n1 >= K // 2 - 1 and n0 >= K // 2 - 1, (n0, n1)
    # the calls did something: every instance has a status, most are solved, and both problems of the extended controller were used
    st = np.concatenate([got[c["status"]] for c in calls])
    assert st.min() >= 0 and (st == 0).mean() > 0.5
    if which == "extended":
        g = got[calls[0]["variant"]]
        assert (got[calls[0]["iters"]][g == 0] > 0).any() and (got[calls[0]["iters"]][g == 1] > 0).any()
    # with the second lane off: one lane, the same numbers
    hip_lib.set_call_overlap(h, False)
    try:
        off, _, ((m0, m1), waits_off) = run(hip_lib, h, bufs, calls, fenced=False)
    finally:
        hip_lib.set_call_overlap(h, True)
    same(off, want)
    assert (m0, m1, waits_off) == (K, 0, 0)


def test_dependent_chain_stays_in_call_order(hip_lib, torch, plain):
    """call k + 1 takes call k's x_nom0 buffer as its x_k: every call conflicts with the one before it and stays on its lane"""
    h = plain[0]._handle
    K = 16
    bufs = Buffers(torch)
    X, R = states(7)
    r = bufs.put("r", R)
    calls, x = [], bufs.put("x", X)
    for k in range(K):
        c = {"x_k": x, "ref": r, **bufs.outputs(f"c{k}")}
        calls.append(c)
        x = c["x_nom0"]
    hip_lib.set_call_overlap(h, True)
    got, _, ((n0, n1), waits) = run(hip_lib, h, bufs, calls, fenced=False)
    want, _, _ = run(hip_lib, h, bufs, calls, fenced=True)
    same(got, want)
    print(f"chain: calls per lane ({n0}, {n1}), cross-lane waits {waits}")
    assert n0 + n1 == K and (min(n0, n1) == 0 or waits > 0)
    assert (got[calls[-1]["status"]] == 0).mean() > 0.5          # the last link solved real states, not the NaN fill


def test_waw_war_and_a_call_that_depends_on_both_lanes(hip_lib, torch, plain):
    h = plain[0]._handle
    bufs = Buffers(torch)
    (X1, R1), (X2, R2), (X3, R3) = states(11), states(12), states(13)
    x1, r1, x2, r2, x3, r3 = (bufs.put(n, a) for n, a in (("x1", X1), ("r1", R1), ("x2", X2), ("r2", R2), ("x3", X3), ("r3", R3)))
    p, q, s = bufs.outputs("p"), bufs.outputs("q"), bufs.outputs("s")
    calls = [
        {"x_k": x1, "ref": r1, **p},                         # lane A
        {"x_k": x2, "ref": r2, **q},                         # independent: lane B
        {"x_k": p["x_nom0"], "ref": r1, **q},                # RAW on the first call, WAW on the second: behind both
        {"x_k": x3, "ref": r3, **q},                         # WAW: same outputs, other inputs -- the last writer's numbers stay
        {"x_k": x3, "ref": r3, **s},
        {"x_k": x2, "ref": r2, **{**p, "x_nom0": x3}},      # WAR: writes its x_nom0 (= X2) into the buffer the two calls before it read
    ]
    hip_lib.set_call_overlap(h, True)
    got, _, ((n0, n1), waits) = run(hip_lib, h, bufs, calls, fenced=False)
    want, _, _ = run(hip_lib, h, bufs, calls, fenced=True)
    same(got, want)
    print(f"hazards: calls per lane ({n0}, {n1}), cross-lane waits {waits}")
    assert n0 + n1 == len(calls)
    assert waits >= 1                                        # the third call
    # (fixed initial state: x_nom0 is x_k) the WAR call did overwrite x3, after its readers had used the old contents
    okw, ok = got[p["status"]] == 0, got[s["status"]] == 0
    assert okw.mean() > 0.5 and np.allclose(got[x3][okw], X2[okw], rtol=0, atol=1e-9) and np.abs(X2 - X3)[okw].max() > 1e-3
    assert ok.mean() > 0.5 and np.allclose(got[s["x_nom0"]][ok], X3[ok], rtol=0, atol=1e-9)
    with_overlap = got
    hip_lib.set_call_overlap(h, False)
    try:
        off, _, ((m0, m1), _) = run(hip_lib, h, bufs, calls, fenced=False)
    finally:
        hip_lib.set_call_overlap(h, True)
    same(off, with_overlap)
    assert (m0, m1) == (len(calls), 0)


def test_other_entry_points_join_the_lanes(hip_lib, torch, plain):
    """device-pointer calls followed directly by the closed loop, by a host-pointer determine_packet and by tmpc_get_solve_ticks"""
    mpc, w = plain
    h = mpc._handle
    from LinearMPCOverNetworks import montecarlo
    bufs = Buffers(torch)
    calls = independent_calls(bufs, 6, with_variant=False)
    nb, T = 64, 20
    th, ga, dist = montecarlo.draw_realisations(nb, T, w["w_bound"], seed=3)
    ref = np.where(np.arange(T) < T // 2, 0.5, -0.5)

    def closed_loop():
        out = mpc.run_closed_loop(np.full(nb, 0.3), ref, th, ga, dist)
        return {k: np.asarray(out[k]) for k in ("err2", "x_final", "tube_violations", "not_optimal", "iters_sum")}

    def packet():
        pk = mpc.determine_packet(S[5, :NX], S[5, NX:], 0)
        assert pk["U_t"] is not None
        return {"U_t": np.asarray(pk["U_t"], dtype=np.float64)}

    hip_lib.set_call_overlap(h, True)
    for after in (closed_loop, packet):
        got, extra, ((n0, n1), _) = run(hip_lib, h, bufs, calls, fenced=False, after=after)
        want, extra_ref, _ = run(hip_lib, h, bufs, calls, fenced=True, after=after)
        same(got, want)
        same(extra, extra_ref)
        assert n0 + n1 == len(calls) and n1 >= 2
    # per-solve ticks are those of the LAST call, whichever lane it ran on: one positive count per instance, and the numbers of the
    # calls are what they are without the timing
    L = hip_lib.lib()
    assert L.tmpc_set_solve_timing(h.ptr, 1) == 0
    try:
        for last in (len(calls), len(calls) - 1):            # the last call on either lane
            ticks = np.zeros(B, np.int64)

            def get_ticks():
                assert L.tmpc_get_solve_ticks(h.ptr, B, ticks.ctypes.data) == 0, h.error()
                return {"n": np.array([(ticks > 0).sum()])}
            got, extra, (lanes, _) = run(hip_lib, h, bufs, calls[:last], fenced=False, after=get_ticks)
            assert extra["n"][0] == B, (extra, lanes)
            for k in want:
                if int(k.split(".")[0][1:]) < last:
                    assert np.array_equal(got[k], want[k], equal_nan=True), k
    finally:
        assert L.tmpc_set_solve_timing(h.ptr, 0) == 0


def test_kernel_ms_total_is_busy_time(hip_lib, torch, plain):
    h = plain[0]._handle
    K = 32
    bufs = Buffers(torch)
    calls = independent_calls(bufs, 8, with_variant=False)
    bufs.reset()
    hip_lib.set_call_overlap(h, True)
    for c in calls:                                          # warm-up: the second lane exists, the clocks are up
        bufs.solve(hip_lib, h, c)
    hip_lib.synchronize(h)
    hip_lib.kernel_ms_total(h, reset=True)
    hip_lib.lane_counters(h, reset=True)
    t0 = time.perf_counter()
    for k in range(K):
        bufs.solve(hip_lib, h, calls[k % len(calls)])
    hip_lib.synchronize(h)
    wall_ms = (time.perf_counter() - t0) * 1e3
    total, n = hip_lib.kernel_ms_total(h, reset=True)
    (n0, n1), _ = hip_lib.lane_counters(h)
    print(f"overlapped: {K} calls, busy total {total:.3f} ms, wall {wall_ms:.3f} ms, calls per lane ({n0}, {n1})")
    assert n == K and n0 + n1 == K and min(n0, n1) >= K // 2 - 1
    # the busy time of the handle lies inside the fenced wall time (a few percent for the two fence calls' own time stamps)
    assert 0.0 < total <= 1.05 * wall_ms, (total, wall_ms)
    # one lane: every call adds its own start-to-end time, as before (a float32 sum of K positive terms: relative error < K 2^-24)
    hip_lib.set_call_overlap(h, False)
    try:
        own = []
        for k in range(K):
            bufs.solve(hip_lib, h, calls[k % len(calls)])
            own.append(hip_lib.last_kernel_ms(h))
        total1, n = hip_lib.kernel_ms_total(h, reset=True)
    finally:
        hip_lib.set_call_overlap(h, True)
    print(f"one lane: busy total {total1:.4f} ms, sum of the calls' own times {sum(own):.4f} ms")
    assert n == K and min(own) > 0
    assert abs(total1 - sum(own)) <= 1e-5 * sum(own), (total1, sum(own))


def test_more_calls_than_timing_pairs(hip_lib, torch, plain):
    """tmpc_kernel_ms_total tracks 4096 calls between resets; a server that never resets goes on beyond them.  The hazard records of
    those calls use the lanes' own end events: independent calls still alternate, dependent ones still wait."""
    h = plain[0]._handle
    b = 256
    bufs = Buffers(torch)
    sets = []
    for k in range(4):
        X, R = states(300 + k, b)
        sets.append({"x_k": bufs.put(f"c{k}.x", X), "ref": bufs.put(f"c{k}.r", R), **bufs.outputs(f"c{k}", b)})
    calls = [sets[k % 4] for k in range(4200)]
    # ... then a chain through x_nom0 that starts on one lane's output and writes into the other's
    tail = [{"x_k": sets[0]["x_nom0"], "ref": sets[0]["ref"], **sets[1]}, {"x_k": sets[1]["x_nom0"], "ref": sets[1]["ref"], **sets[2]},
            {"x_k": sets[2]["x_nom0"], "ref": sets[2]["ref"], **sets[3]}]
    calls = calls + tail

    def run_b(fenced):
        bufs.reset()
        hip_lib.synchronize(h)
        hip_lib.lane_counters(h, reset=True)
        for c in calls:
            bufs.solve(hip_lib, h, c, b)
            if fenced:
                hip_lib.synchronize(h)
        hip_lib.synchronize(h)
        return bufs.snapshot(), hip_lib.lane_counters(h)

    hip_lib.set_call_overlap(h, True)
    hip_lib.kernel_ms_total(h, reset=True)
    try:
        got, ((n0, n1), waits) = run_b(False)
        _, tracked = hip_lib.kernel_ms_total(h, reset=False)
        want, _ = run_b(True)
    finally:
        hip_lib.kernel_ms_total(h, reset=True)
    same(got, want)
    print(f"beyond the timing pairs: calls per lane ({n0}, {n1}), cross-lane waits {waits}, calls tracked {tracked}")
    assert tracked == 4096 and n0 + n1 == len(calls) and min(n0, n1) > 1000
    assert (got[sets[3]["status"]] == 0).mean() > 0.5
