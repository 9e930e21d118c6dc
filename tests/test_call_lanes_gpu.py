"""Up to four launch lanes per device handle (include/tmpc.h: tmpc_set_call_lanes; csrc/tmpc_hazard.hpp has the policy,
tests/test_elastic_policy.py checks it on the host).  Every check compares BIT FOR BIT with the same calls on a two-lane handle, fenced by
tmpc_synchronize; the outputs start as NaN / -1, and a call's inputs are another call's outputs where order matters: an instance that nobody
solved, or one solved before its input was there, shows as a mismatch.  The handles under test are created with TMPC_CALL_LANES=4 whatever the
library's default is.  Cart-pole N = 10, the 600-state fixture, calls of two instances per resident wave."""
import os
import re
import time

import numpy as np
import pytest

import common
from test_call_overlap import ARGS, NX, NU, N, S, Buffers, same, states

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def make(env, extended=False):
    """a device handle created under the environment `env` (the lane count is read once, at tmpc_create)"""
    keys = ("TMPC_CALL_LANES",)
    old = {k: os.environ.pop(k, None) for k in keys}
    os.environ.update(env)
    try:
        return common.make_mpc("cartpole", N, True, extended=extended, create=True)[0]
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


FOUR = {"TMPC_CALL_LANES": "4"}


@pytest.fixture(scope="module")
def four(hip_lib):
    return make(FOUR)


@pytest.fixture(scope="module")
def ref(hip_lib):
    return make({"TMPC_CALL_LANES": "2"})


@pytest.fixture(scope="module")
def grid(hip_lib, torch, four):
    """(CUs, waves per workgroup, the batch of two instances per resident wave) of the handle's kernel on this card"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    name = hip_lib.kernel_name(four._handle, 0)
    wpb = int(re.search(r",\s*(\d+)>$", name).group(1))
    thr = 2 * n_cu * wpb
    assert hip_lib.get_call_lanes(four._handle) == 4
    return n_cu, wpb, thr


def run(hip, h, bufs, calls, fenced, b, after=None):
    bufs.reset()
    hip.synchronize(h)
    hip.lane_counters_n(h, reset=True)
    for c in calls:
        bufs.solve(hip, h, c, b)
        if fenced:
            hip.synchronize(h)
    extra = after() if after else None
    hip.synchronize(h)
    return bufs.snapshot(), extra, hip.lane_counters_n(h)


def independent(bufs, K, b, with_variant=False, seed=100):
    calls = []
    for k in range(K):
        X, R = states(seed + k, b)
        c = {"x_k": bufs.put(f"c{k}.x", X), "ref": bufs.put(f"c{k}.r", R), **bufs.outputs(f"c{k}", b, traj=(k % 4 == 0))}
        if with_variant:
            c["variant"] = bufs.put(f"c{k}.g", np.random.default_rng(200 + k).integers(0, 2, b).astype(np.uint8))
        calls.append(c)
    return calls


def solved(got, calls):
    st = np.concatenate([got[c["status"]] for c in calls])
    assert st.min() >= 0 and (st == 0).mean() > 0.5


@pytest.mark.parametrize("which", ["plain", "extended"])
def test_burst_on_four_lanes(hip_lib, torch, four, ref, grid, which):
    """16 independent calls: they rotate over four lanes, nothing waits; the extended controller's calls are two filtered launches each"""
    n_cu, wpb, thr = grid
    ext = which == "extended"
    h4, href = (make(FOUR, extended=True), make({"TMPC_CALL_LANES": "2"}, extended=True)) if ext else (four, ref)
    K = 16
    bufs = Buffers(torch)
    calls = independent(bufs, K, thr, with_variant=ext)
    want, _, _ = run(hip_lib, href._handle, bufs, calls, True, thr)
    got, _, (per_lane, waits) = run(hip_lib, h4._handle, bufs, calls, False, thr)
    same(got, want)
    solved(got, calls)
    print(f"{which}: calls per lane {per_lane}, cross-lane waits {waits}")
    assert sum(per_lane) == K and waits == 0
    # a lane is created by the first call that finds every existing lane busy; from then on the calls rotate
    assert min(per_lane) >= K // 4 - 1, per_lane
    # the two-entry counter goes by the parity of the lane changes: calls in rotation alternate between its entries
    (n0, n1), _ = hip_lib.lane_counters(h4._handle)
    assert n0 + n1 == K and min(n0, n1) >= K // 2 - 1, (n0, n1)
    if ext:
        g = got[calls[0]["variant"]]
        assert (got[calls[0]["iters"]][g == 0] > 0).any() and (got[calls[0]["iters"]][g == 1] > 0).any()
    # two lanes and one lane on the same handle: the same numbers
    for lanes in (2, 1):
        hip_lib.set_call_lanes(h4._handle, lanes)
        try:
            again, _, (pl, _) = run(hip_lib, h4._handle, bufs, calls, False, thr)
        finally:
            hip_lib.set_call_lanes(h4._handle, 4)
        same(again, want)
        assert sum(pl) == K and sum(pl[lanes:]) == 0


def test_hazards_on_four_lanes(hip_lib, torch, four, ref, grid):
    n_cu, wpb, b = grid
    bufs = Buffers(torch)
    X = [states(10 + k, b) for k in range(5)]
    x = [bufs.put(f"x{k}", a[0]) for k, a in enumerate(X)]
    r = [bufs.put(f"r{k}", a[1]) for k, a in enumerate(X)]
    o = [bufs.outputs(f"o{k}", b) for k in range(6)]
    calls = [
        {"x_k": x[0], "ref": r[0], **o[0]},                          # four independent calls: a lane each
        {"x_k": x[1], "ref": r[1], **o[1]},
        {"x_k": x[2], "ref": r[2], **o[2]},
        {"x_k": x[3], "ref": r[3], **o[3]},
        # reads the first call's x_nom0 (RAW), writes the second's u_nom and the third's status (WAW): behind three lanes
        {"x_k": o[0]["x_nom0"], "ref": r[0], **{**o[4], "u_nom": o[1]["u_nom"], "status": o[2]["status"]}},
        {"x_k": x[4], "ref": r[4], **o[3]},                          # WAW on the fourth call: the last writer's numbers stay
        {"x_k": x[1], "ref": r[1], **{**o[5], "x_nom0": x[4]}},      # WAR: overwrites the input of the call before it
    ]
    # ... and a dependent chain through x_nom0 behind them
    xk = o[4]["x_nom0"]
    for k in range(4):
        c = {"x_k": xk, "ref": r[0], **bufs.outputs(f"chain{k}", b)}
        calls.append(c)
        xk = c["x_nom0"]
    want, _, _ = run(hip_lib, ref._handle, bufs, calls, True, b)
    got, _, (per_lane, waits) = run(hip_lib, four._handle, bufs, calls, False, b)
    same(got, want)
    print(f"hazards: calls per lane {per_lane}, cross-lane waits {waits}")
    assert sum(per_lane) == len(calls) and waits >= 1
    assert (got[calls[-1]["status"]] == 0).mean() > 0.5          # the chain's last link solved real states, not the NaN fill
    ok = got[o[5]["status"]] == 0
    assert ok.mean() > 0.5 and np.allclose(got[x[4]][ok], X[1][0][ok], rtol=0, atol=1e-9)      # (fixed initial state: x_nom0 is x_k)


def test_other_entry_points_behind_four_lanes(hip_lib, torch, four, ref, grid):
    """device-pointer calls followed directly by the closed loop, by a host-pointer determine_packet and by tmpc_get_solve_ticks"""
    n_cu, wpb, b = grid
    from LinearMPCOverNetworks import montecarlo
    w = common.workload("cartpole")
    bufs = Buffers(torch)
    calls = independent(bufs, 7, b)
    nb, T = 64, 10
    th, ga, dist = montecarlo.draw_realisations(nb, T, w["w_bound"], seed=3)
    rseq = np.where(np.arange(T) < T // 2, 0.5, -0.5)

    def after_on(mpc):
        def closed_loop():
            out = mpc.run_closed_loop(np.full(nb, 0.3), rseq, th, ga, dist)
            return {k: np.asarray(out[k]) for k in ("err2", "x_final", "tube_violations", "not_optimal", "iters_sum")}

        def packet():
            pk = mpc.determine_packet(S[5, :NX], S[5, NX:], 0)
            assert pk["U_t"] is not None
            return {"U_t": np.asarray(pk["U_t"], dtype=np.float64)}
        return closed_loop, packet

    for a4, aref in zip(after_on(four), after_on(ref)):
        want, extra_ref, _ = run(hip_lib, ref._handle, bufs, calls, True, b, after=aref)
        got, extra, (per_lane, _) = run(hip_lib, four._handle, bufs, calls, False, b, after=a4)
        same(got, want)
        same(extra, extra_ref)
        assert sum(per_lane) == len(calls) and sum(1 for n in per_lane if n > 0) >= 3, per_lane
    L, h = hip_lib.lib(), four._handle
    assert L.tmpc_set_solve_timing(h.ptr, 1) == 0
    try:
        for last in (len(calls), len(calls) - 1, len(calls) - 2):            # the last call on three different lanes
            ticks = np.zeros(b, np.int64)

            def get_ticks():
                assert L.tmpc_get_solve_ticks(h.ptr, b, ticks.ctypes.data) == 0, h.error()
                return {"n": np.array([(ticks > 0).sum()])}
            got, extra, (per_lane, _) = run(hip_lib, h, bufs, calls[:last], False, b, after=get_ticks)
            assert extra["n"][0] == b, (extra, per_lane)
            for k in want:
                if int(k.split(".")[0][1:]) < last:
                    assert np.array_equal(got[k], want[k], equal_nan=True), k
    finally:
        assert L.tmpc_set_solve_timing(h.ptr, 0) == 0


def test_kernel_ms_total_is_busy_time_on_four_lanes(hip_lib, torch, four, grid):
    n_cu, wpb, b = grid
    h = four._handle
    K = 32
    bufs = Buffers(torch)
    calls = independent(bufs, 8, b)
    bufs.reset()
    for c in calls:                                          # warm-up: the lanes exist, the clocks are up
        bufs.solve(hip_lib, h, c, b)
    hip_lib.synchronize(h)
    hip_lib.kernel_ms_total(h, reset=True)
    hip_lib.lane_counters_n(h, reset=True)
    t0 = time.perf_counter()
    for k in range(K):
        bufs.solve(hip_lib, h, calls[k % len(calls)], b)
    hip_lib.synchronize(h)
    wall_ms = (time.perf_counter() - t0) * 1e3
    total, n = hip_lib.kernel_ms_total(h, reset=True)
    per_lane, _ = hip_lib.lane_counters_n(h)
    print(f"four lanes: {K} calls, busy total {total:.3f} ms, wall {wall_ms:.3f} ms, calls per lane {per_lane}")
    assert n == K and sum(per_lane) == K and min(per_lane) >= K // 4 - 1
    assert 0.0 < total <= 1.05 * wall_ms, (total, wall_ms)
    # one lane: every call adds its own start-to-end time (a float32 result of K positive terms: relative error < K 2^-24)
    hip_lib.set_call_lanes(h, 1)
    try:
        own = []
        for k in range(K):
            bufs.solve(hip_lib, h, calls[k % len(calls)], b)
            own.append(hip_lib.last_kernel_ms(h))
        total1, n = hip_lib.kernel_ms_total(h, reset=True)
    finally:
        hip_lib.set_call_lanes(h, 4)
    print(f"one lane: busy total {total1:.4f} ms, sum of the calls' own times {sum(own):.4f} ms")
    assert n == K and min(own) > 0
    assert abs(total1 - sum(own)) <= 1e-5 * sum(own), (total1, sum(own))
