"""Time-resolved records of the device closed loops and their ensemble statistics on the card (include/tmpc.h: tmpc_mc_set_series,
tmpc_mc_get_series, tmpc_mc_series_stats, tmpc_series_stats; csrc/tmpc_mc_step.hpp, csrc/tmpc_series.hip).

Bands.  Where the same arithmetic runs twice, bytes.  The reduction against its numpy twin: every integer table, e_max and e_q by bytes;
e_sum within 2 n 2^-52 sum |e| (tests/wavesim/series_case.py: e_sum_bound).  The device loop against the host loop: the project's band on
states between the two loops is delta = 1e-8 (x_final in tests/test_closed_loop.py::test_device_resident_loop_equals_host_loop); two
states within delta per component are within sqrt(nx) delta in norm, so their squared distances e = |x - r|^2 to one reference differ by
at most (2 sqrt(e_host) + sqrt(nx) delta) sqrt(nx) delta.

The loops: the cart-pole at N = 10 and the double integrator, B = 70 trajectories (more than one workgroup of four waves, and no multiple
of it), T = 40 steps, every trajectory with its own Gilbert-Elliott channel -- the set-up of tests/test_channel_gpu.py."""
import os
import re
import runpy
import sys

import numpy as np
import pytest

import common
from LinearMPCOverNetworks import _native, montecarlo, workloads
from test_stepped_loop_api import E_INVALID

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "wavesim"))
import series_case  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB, T = 70, 40
ALL_LOST, NEVER_LOST = 1, 2
LINK = ("lost_up", "lost_down", "max_gap", "overrun")
KEYS = ("err2", "tube_violations", "not_optimal", "x_final", "consistent", "iters_sum") + LINK
FLAGS = ("lost_up", "lost_down", "adopted", "tube", "not_optimal", "overrun")
SEED = {("cartpole", False): 23, ("cartpole", True): 23, ("double_integrator", False): 41}
CASES = [("cartpole", False), ("cartpole", True), ("double_integrator", False)]
DELTA = 1e-8


def _channel(nb=NB):
    rng = np.random.default_rng(17)
    ch = dict(p_gb=rng.uniform(0.05, 0.5, nb), p_bg=rng.uniform(0.1, 0.9, nb), e_g=rng.uniform(0.0, 0.2, nb), e_b=rng.uniform(0.5, 1.0, nb))
    for b, par in ((0, (0.0, 0.5, 0.3, 0.9)), (ALL_LOST, (1.0, 0.0, 0.1, 1.0)), (NEVER_LOST, (0.4, 0.3, 0.0, 0.0))):
        for k, v in zip(("p_gb", "p_bg", "e_g", "e_b"), par):
            ch[k][b] = v
    return ch


CH = _channel()
_CASE = {}


def _case(name, extended):
    """Controller, realisations and, computed once and left alone: the device run with its record (launch per step, cold) and the HOST loop
    with its record (numpy state machines and the numpy channel around the device solver, whose iterations it records)."""
    key = (name, extended)
    if key not in _CASE:
        if name == "cartpole":
            mpc, w = common.make_mpc("cartpole", 10, True, extended=extended, create=True)
            ref = np.where(np.arange(T) < T // 2, 0.5, -0.3)
        else:
            mpc, w = workloads.make_controller("double_integrator", 10, fixed_initial_state=False)
            ref = np.where(np.arange(T) < T // 2, 2.0, -1.2)
        th, ga, dist = montecarlo.draw_realisations(NB, T, w["w_bound"], seed=SEED[key])
        c = dict(mpc=mpc, w=w, ref=ref, th=th, ga=ga, dist=dist, extended=extended)

        def packets(*a):
            return mpc.determine_packets(*a) + (mpc.last_iters,)
        c["host"] = montecarlo.run_remote_tube_mpc(packets, w["A"], w["B"], mpc.get_steady_state_controller_gain(), mpc.get_ancillary_controller_gain(),
                                                   mpc._N, mpc._Z, None, ref, th, ga, dist, extended=extended, channel=CH, series=True)
        # the seeds are those of the channel tests: every solve of the host loop is optimal, so its integers are exact
        assert np.all(c["host"]["not_optimal"] == 0), (key, c["host"]["not_optimal"])
        c["dev"] = _run(c, fused="off", series=True)
        _CASE[key] = c
    return _CASE[key]


def _run(c, p_loss=None, channel=CH, **kw):
    return c["mpc"].run_closed_loop(p_loss, c["ref"], c["th"], c["ga"], c["dist"], extended=c["extended"], channel=channel, **kw)


def _same(a, b, keys=KEYS):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def _same_series(a, b, rows=slice(None)):
    assert a["series"]["e"][:, rows].tobytes() == b["series"]["e"][:, rows].tobytes()
    assert a["series"]["word"][:, rows].tobytes() == b["series"]["word"][:, rows].tobytes()


def _identities(out, rows, N, steps=None, stopped=False):
    """The record of the trajectories `rows` against the outputs of the very loop that wrote it."""
    s = out["series"]
    steps = s["e"].shape[0] if steps is None else steps
    acc = np.zeros(s["e"].shape[1])
    for t in range(steps):
        acc += s["e"][t]                                                       # the loop's order: step by step
    if not stopped:                                                            # (a stopped trajectory's err2 is NaN)
        assert acc[rows].tobytes() == np.asarray(out["err2"])[rows].tobytes()
    extra = 1 if stopped else 0                                                # the infeasible solve is counted, and takes no step
    assert np.array_equal(s["not_optimal"].sum(axis=0)[rows] + extra, out["not_optimal"][rows])
    for key, flag in (("lost_up", "lost_up"), ("lost_down", "lost_down"), ("overrun", "overrun"), ("tube_violations", "tube")):
        assert np.array_equal(s[flag].sum(axis=0)[rows], out[key][rows]), key
    assert np.array_equal(s["age"].max(axis=0)[rows], out["max_gap"][rows])
    if not stopped:
        assert np.array_equal(s["iters"].sum(axis=0)[rows], out["iters_sum"][rows])
    assert np.array_equal(s["overrun"], s["alive"] & (s["age"] >= N))
    assert s["word"].dtype == np.uint32 and not np.any(s["word"] & np.uint32(0x80))


def _e_band(e_host, nx):
    return (2.0 * np.sqrt(e_host) + np.sqrt(nx) * DELTA) * np.sqrt(nx) * DELTA


# ------------------------------------------------------------------------------------------------ 5: the reduction's edge shapes
def test_reduction_edge_shapes(hip_lib):
    """T = 3; interleaved groups of 0, 1, 2, 63, 64, 65, 255, 256, 257 and 2049 members (3012 grouped trajectories), seven members of no
    group and a group of twenty dead words: tests/wavesim/series_case.py::edge_record."""
    e, word, group, G = series_case.edge_record()
    q = series_case.QUANTILES
    ref = montecarlo.series_stats(e, word, group, q, G=G)
    dev = _native.series_stats(e, word, group, q, G=G)
    again = _native.series_stats(e, word, group, q, G=G)
    bound = series_case.e_sum_bound(e, word, group, G)
    fin = np.isfinite(bound)
    gap = np.abs(dev["e_sum"][fin] - ref["e_sum"][fin])
    print(f"   {word.shape[1]} trajectories, {G} groups of {ref['n_alive'][0].tolist()}: kernel {dev['kernel_ms']:.3f} ms; "
          f"max |e_sum - twin| / bound = {np.max(gap[bound[fin] > 0] / bound[fin][bound[fin] > 0]):.3f}")
    for k in series_case.EXACT:
        assert dev[k].dtype == ref[k].dtype and dev[k].tobytes() == ref[k].tobytes(), k
    assert np.all(gap <= bound[fin]) and np.array_equal(dev["e_sum"][~fin], ref["e_sum"][~fin]) and (~fin).sum() > 0
    for k in series_case.EXACT + ("e_sum",):
        assert dev[k].tobytes() == again[k].tobytes(), k
    assert ref["n_alive"][0].tolist() == list(series_case.SIZES) + [0] and ref["n_nan"][2].sum() > 0
    assert np.isnan(dev["e_q"][:, G - 1]).all() and np.isnan(dev["e_max"][:, 0]).all() and not dev["e_sum"][:, 0].any()
    # one group of everybody, sixteen quantiles, and none
    q16 = q + tuple(np.linspace(0.01, 0.99, 11))
    for qq in (q16, ()):
        ref1, dev1 = montecarlo.series_stats(e, word, None, qq, G=1), _native.series_stats(e, word, None, qq)
        for k in series_case.EXACT:
            assert dev1[k].tobytes() == ref1[k].tobytes(), k
        b1 = series_case.e_sum_bound(e, word, np.zeros(word.shape[1], np.int32), 1)
        f1 = np.isfinite(b1)
        assert np.all(np.abs(dev1["e_sum"][f1] - ref1["e_sum"][f1]) <= b1[f1]) and np.array_equal(dev1["e_sum"][~f1], ref1["e_sum"][~f1])


# ------------------------------------------------------------------------------------------------ 6: identities on the device
@pytest.mark.parametrize("name,extended", CASES)
def test_device_record_adds_up_to_the_runs_own_outputs(hip_lib, name, extended):
    c = _case(name, extended)
    dev = c["dev"]
    assert dev["series"]["e"].shape == dev["series"]["word"].shape == (T, NB) and dev["series"]["alive"].all()
    _identities(dev, np.arange(NB), c["mpc"]._N)
    s = dev["series"]
    assert s["age"][:, ALL_LOST].tolist() == list(range(T)) and not s["age"][:, NEVER_LOST].any() and s["adopted"][0].all()
    assert s["lost_up"].sum() > 0 and s["overrun"].sum() > 0 and s["iters"].max() > 0


# ------------------------------------------------------------------------------------------------ 7: device against host loop
@pytest.mark.parametrize("name,extended", CASES)
def test_device_record_equals_the_host_loops(hip_lib, name, extended):
    c = _case(name, extended)
    d, h = c["dev"]["series"], c["host"]["series"]
    differ = np.argwhere(d["word"] != h["word"])
    assert differ.size == 0, (differ[:5], [{k: (d[k][t, b], h[k][t, b]) for k in ("iters", "age") + FLAGS} for t, b in differ[:3]])
    band = _e_band(h["e"], c["mpc"]._nx)
    gap = np.abs(d["e"] - h["e"])
    print(f"   {name}, extended = {extended}: max |e_dev - e_host| = {gap.max():.2e} (largest e {h['e'].max():.2e}), max gap / band = {np.max(gap / band):.2e}")
    assert np.all(gap <= band)


# ------------------------------------------------------------------------------------------------ 8: the loop forms
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("name,extended", CASES)
def test_loop_forms_record_the_same(hip_lib, name, extended, warm):
    """A recording loop runs per time step whatever tmpc_mc_set_fused says (the fused kernels carry no recording code):
    loop_mode 0 with fused on and off, the same bytes -- and the loop's other outputs are those of the fused run that does not record."""
    c = _case(name, extended)
    off = c["dev"] if not warm else _run(c, fused="off", warm_start=True, series=True)
    on = _run(c, fused="on", warm_start=warm, series=True)
    assert off["loop_mode"] == 0 and on["loop_mode"] == 0
    _same_series(on, off)
    _same(on, off)
    plain = _run(c, fused="on", warm_start=warm)
    assert plain["loop_mode"] == (2 if extended else 1) and "series" not in plain
    _same(plain, on)
    if warm:                                                                   # fewer iterations, the same flags and ages
        cold = c["dev"]["series"]
        assert np.array_equal(on["series"]["word"] & np.uint32(0xfff000ff), cold["word"] & np.uint32(0xfff000ff))
        assert on["series"]["iters"].sum() < cold["iters"].sum()
        _identities(on, np.arange(NB), c["mpc"]._N)


def test_block_path_records_like_the_wave_path(hip_lib):
    mpc, w = common.make_mpc("cartpole", 10, True, create=True)
    try:
        c = dict(_case("cartpole", False), mpc=mpc)
        mpc.set_kernel_path("block")
        blk = _run(c, series=True)
        assert blk["loop_mode"] == 0 and mpc.get_kernel_path() == "block"
        _identities(blk, np.arange(NB), mpc._N)
        d, v = blk["series"], c["dev"]["series"]
        differ = np.argwhere(d["word"] != v["word"])
        print(f"   block against wave: {len(differ)} words differ; iterations block {d['iters'].mean():.2f}, wave {v['iters'].mean():.2f} per solve")
        assert differ.size == 0, [{k: (d[k][t, b], v[k][t, b]) for k in ("iters", "age") + FLAGS} for t, b in differ[:3]]
        gap = np.abs(d["e"] - v["e"])
        print(f"   max |e_block - e_wave| = {gap.max():.2e}")
        assert np.all(gap <= _e_band(v["e"], mpc._nx))
    finally:
        mpc._close()


# ------------------------------------------------------------------------------------------------ 9: session and plants
@pytest.mark.parametrize("extended", [False, True])
def test_session_fed_a_recorded_trajectory_records_the_runs_bytes(hip_lib, extended):
    """The construction of tests/test_stepped_loop.py: trajectory k of a tmpc_mc_run, recorded, is fed to trajectory k of a session step
    by step -- the same record byte for byte (mc_session_kernel against mc_step_kernel).  A setter call while the session is open is
    refused and leaves the record intact."""
    c = _case("cartpole", extended)
    mpc, w = c["mpc"], c["w"]
    A, B = np.asarray(w["A"], dtype=np.float64), np.asarray(w["B"], dtype=np.float64)
    h, L = mpc._handle, _native.lib()
    for k in (ALL_LOST, 7, 69):
        run = _run(c, fused="off", capture=k, series=True)
        _same_series(run, c["dev"])
        x = np.zeros((NB, mpc._nx))
        with mpc.open_closed_loop(None, c["ref"], c["th"], c["ga"], extended=extended, channel=CH, series=True) as s:
            for t in range(T):
                if t == 5:
                    assert L.tmpc_mc_set_series(h.ptr, 0) == E_INVALID and "stepped closed loop is open" in h.error()
                x[k] = run["x_traj"][t]
                u = s.step(x)
                x = x @ A.T + u @ B.T + c["dist"][:, t]
        ses = s.stats
        assert ses["steps"] == T and ses["loop_mode"] == 0
        _same_series(ses, run, rows=slice(k, k + 1))
        assert ses["series"]["alive"].all()
        _identities(ses, np.arange(NB), mpc._N)


def test_session_closed_early_has_zero_rows(hip_lib):
    c = _case("cartpole", False)
    mpc, w = c["mpc"], c["w"]
    A, B = np.asarray(w["A"], dtype=np.float64), np.asarray(w["B"], dtype=np.float64)
    k = 13
    x = np.zeros((NB, mpc._nx))
    with mpc.open_closed_loop(None, c["ref"], c["th"], c["ga"], channel=CH, series=True) as s:
        for t in range(k):
            u = s.step(x)
            x = x @ A.T + u @ B.T + c["dist"][:, t]
    ses = s.stats
    assert ses["steps"] == k and ses["series"]["e"].shape == (T, NB)
    assert ses["series"]["alive"][:k].all() and not ses["series"]["word"][k:].any() and not ses["series"]["e"][k:].any()
    _identities(ses, np.arange(NB), mpc._N, steps=k)
    stats = _native.mc_series_stats(mpc._handle, q=(0.5,))
    assert stats["n_alive"][:, 0].tolist() == [NB] * k + [0] * (T - k) and np.isnan(stats["e_q"][k:]).all()


def test_nominal_plant_family_records_the_runs_bytes(hip_lib):
    c = _case("cartpole", False)
    w = c["w"]
    lin = montecarlo.plant_family("linear", A=np.tile(w["A"], (NB, 1, 1)), B=np.tile(w["B"], (NB, 1, 1)))
    fam = _run(c, plant=lin, series=True)
    assert fam["loop_mode"] == 0
    gap = np.abs(fam["series"]["e"] - c["dev"]["series"]["e"])
    print(f"   nominal linear family against the loop's own plant: max |e - e| = {gap.max():.2e}, {np.count_nonzero(fam['series']['word'] != c['dev']['series']['word'])} words differ")
    _same_series(fam, c["dev"])
    _identities(fam, np.arange(NB), c["mpc"]._N)


# ------------------------------------------------------------------------------------------------ 10: R-MPC
def test_stopped_rmpc_trajectories_are_not_alive(hip_lib):
    """The scenario of tests/test_channel_gpu.py::test_stopped_rmpc_trajectories_stop_counting."""
    mpc, w = workloads.make_controller("double_integrator", 10, tracking=True)
    try:
        nt = 60
        rng = np.random.default_rng(11)
        x0 = (rng.uniform(-1, 1, (96, 2)) * [7.6, 0.6])[:NB]
        th, ga, dist = montecarlo.draw_realisations(NB, nt, 3.0 * w["w_bound"], seed=5)
        ref = np.where(np.arange(nt) < 30, 6.0, -6.0)
        dev = mpc.run_closed_loop(None, ref, th, ga, dist, x0=x0, channel=CH, series=True)
        s = dev["series"]
        dead = np.isnan(dev["tracking_error"])
        assert 0 < dead.sum() < NB and dev["loop_mode"] == 0
        steps = s["alive"].sum(axis=0)
        assert np.all(steps[~dead] == nt) and np.all(steps[dead] < nt)
        for b in np.flatnonzero(dead):                                         # alive up to the stopping step, nothing from there on
            assert s["alive"][:steps[b], b].all() and not s["word"][steps[b]:, b].any() and not s["e"][steps[b]:, b].any()
        _identities(dev, np.flatnonzero(~dead), mpc._N)
        _identities(dev, np.flatnonzero(dead), mpc._N, stopped=True)
        stats = _native.mc_series_stats(mpc._handle, q=(0.5, 1.0))
        assert np.array_equal(stats["n_alive"][:, 0], s["alive"].sum(axis=1)) and stats["n_alive"][-1, 0] == NB - dead.sum()
        assert not stats["n_nan"].any() and np.array_equal(stats["e_q"][:, 0, 1], stats["e_max"][:, 0])
    finally:
        mpc._close()


# ------------------------------------------------------------------------------------------------ 11: the resident record
def test_resident_reduction_equals_the_stand_alone_one(hip_lib):
    """Loss-rate groups as montecarlo.trajectory_table lays them out (loss-rate-minor: the groups interleave), on the record where the
    loop left it, against tmpc_series_stats on the copied-out arrays: bytes; and both against the numpy twin."""
    c = _case("cartpole", False)
    rates = np.array([0.0, 0.2, 0.4, 0.6, 0.8, 0.3, 0.5])
    pi, _ = montecarlo.trajectory_table(rates, NB // len(rates))
    assert len(pi) == NB and pi[0] != pi[1]
    dev = _run(c, p_loss=rates[pi], channel=None, series=True)
    q = (0.5, 0.95, 1.0)
    res = _native.mc_series_stats(c["mpc"]._handle, group=pi, q=q, G=len(rates))
    alone = _native.series_stats(dev["series"]["e"], dev["series"]["word"], pi, q, G=len(rates))
    twin = montecarlo.series_stats(dev["series"]["e"], dev["series"]["word"], pi, q, G=len(rates))
    for k in series_case.EXACT + ("e_sum",):
        assert res[k].tobytes() == alone[k].tobytes(), k
    for k in series_case.EXACT:
        assert res[k].tobytes() == twin[k].tobytes(), k
    assert np.all(res["n_alive"] == NB // len(rates)) and res["lost_up"][:, 0].sum() == 0 and res["lost_up"][1:, 4].sum() > 0
    assert np.array_equal(res["e_q"][:, :, 2], res["e_max"]) and res["kernel_ms"] > 0.0
    # a getter with another shape is refused, the record stays
    L, h = _native.lib(), c["mpc"]._handle
    assert L.tmpc_mc_get_series(h.ptr, NB, T + 1, None, None) == E_INVALID and L.tmpc_mc_get_series(h.ptr, NB - 1, T, None, None) == E_INVALID
    assert L.tmpc_mc_get_series(h.ptr, NB, T, None, None) == 0
    _same_series(dict(series=_native.mc_get_series(h, NB, T)), dev)


# ------------------------------------------------------------------------------------------------ 12: series off
@pytest.mark.parametrize("name,extended", CASES[:2])
def test_series_off_is_what_it_was(hip_lib, name, extended):
    c = _case(name, extended)
    h, L = c["mpc"]._handle, _native.lib()
    before = _run(c, capture=5, fused="on")
    assert before["loop_mode"] == (2 if extended else 1) and "series" not in before
    assert L.tmpc_mc_get_series(h.ptr, NB, T, None, None) == E_INVALID and "tmpc_mc_set_series" in h.error()
    on = _run(c, capture=5, fused="on", series=True)
    after = _run(c, capture=5, fused="on")
    _same(after, before, KEYS + ("x_traj", "x_nom_traj", "u_traj"))
    _same(on, before, KEYS + ("x_traj", "x_nom_traj", "u_traj"))
    assert after["loop_mode"] == before["loop_mode"] and L.tmpc_mc_get_series(h.ptr, NB, T, None, None) == E_INVALID
    with pytest.raises(RuntimeError, match="kept no per-step record"):
        _native.mc_series_stats(h)


def test_error_over_time_example_runs(hip_lib, capsys, monkeypatch):
    from LinearMPCOverNetworks import polytope_lite as pl
    old = pl.set_lp_backend("hip")           # the examples use the package defaults
    monkeypatch.setattr(sys, "argv", ["error_over_time.py", "--trajectories", "64", "--steps", "60"])
    try:
        runpy.run_path(os.path.join(ROOT, "examples", "error_over_time.py"), run_name="__main__")
    finally:
        pl.set_lp_backend(old)
    out = capsys.readouterr().out
    assert "cart-pole, N = 10: 64 trajectories per channel, 60 steps" in out
    rows = re.findall(r"^ *(\d+) +([0-9.e+-]+) +([0-9.e+-]+) +([0-9.e+-]+) +([0-9.]+) +\| +([0-9.e+-]+) +([0-9.e+-]+) +([0-9.e+-]+) +([0-9.]+)$", out, re.M)
    assert len(rows) >= 10
    for r in rows:
        for m, p95, mx in ((float(r[1]), float(r[2]), float(r[3])), (float(r[5]), float(r[6]), float(r[7]))):
            assert m <= p95 <= mx
    back = re.findall(r"95 % envelope back under ([0-9.e+-]+) from step (\d+|never) \(independent\), (\d+|never) \(bursty\)", out)
    assert len(back) == 1
