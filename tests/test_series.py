"""Time-resolved records of the closed loops and their ensemble statistics (include/tmpc.h: tmpc_mc_set_series, tmpc_mc_get_series,
tmpc_mc_series_stats, tmpc_series_stats), the part that needs no GPU: the numpy twin of the reduction against a per-column Python loop,
the packed word, the host loops' records against the host loops' own sums and counters, every refusal the entry points give before they
touch a device, and the reduction kernel's SOURCE (csrc/tmpc_series.hip) on the host execution model of tests/wavesim under ASan + UBSan
and under MSan against the numpy twin."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import common
import regulator_problems as rp
from LinearMPCOverNetworks import _native, montecarlo, workloads
from LinearMPCOverNetworks.polytope_lite import Polytope
from test_stepped_loop_api import E_DEVICE, E_INVALID

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "wavesim"))
import hostsim  # noqa: E402
import series_case  # noqa: E402

FLAGS = ("lost_up", "lost_down", "adopted", "tube", "not_optimal", "overrun")


# ------------------------------------------------------------------------------------------------ 1: the word and the numpy twin
def test_word_round_trip_and_saturation():
    rng = np.random.default_rng(0)
    n = 500
    f = {k: rng.integers(0, 2, n).astype(bool) for k in ("alive",) + FLAGS}
    iters, age = rng.integers(0, 4096, n), rng.integers(0, 4096, n)
    iters[:4], age[:4] = [0, 4095, 4096, 100000], [4095, 0, 5000, 4096]
    w = montecarlo.pack_series_word(iters=iters, age=age, **f)
    assert w.dtype == np.uint32 and not np.any(w & np.uint32(0x80))            # bit 7 is zero
    back = montecarlo.unpack_series_word(w)
    for k in f:
        assert np.array_equal(back[k], f[k]), k
    assert np.array_equal(back["iters"], np.minimum(iters, 4095)) and np.array_equal(back["age"], np.minimum(age, 4095))
    # the layout of include/tmpc.h, written out
    one = montecarlo.pack_series_word(True, lost_up=1, adopted=1, overrun=1, iters=3, age=2)
    assert int(one) == 0x01 | 0x02 | 0x08 | 0x40 | (3 << 8) | (2 << 20)
    assert int(montecarlo.pack_series_word(False, tube=1, not_optimal=1, lost_down=1, iters=9999, age=9999)) == 0x04 | 0x10 | 0x20 | (4095 << 8) | (4095 << 20)
    hdr = open(os.path.join(common.ROOT, "include", "tmpc.h")).read()
    for name, val in (("ALIVE", "0x01u"), ("LOST_UP", "0x02u"), ("LOST_DOWN", "0x04u"), ("ADOPTED", "0x08u"), ("TUBE", "0x10u"), ("NOT_OPTIMAL", "0x20u"),
                      ("OVERRUN", "0x40u"), ("ITERS_SHIFT", "8"), ("AGE_SHIFT", "20"), ("SATURATE", "4095"), ("MAX_Q", "16")):
        assert any(line.split() == ["#define", "TMPC_SER_" + name, val] for line in hdr.splitlines()), name


def _naive_stats(e, word, group, q, G):
    """Column by column in plain Python: what include/tmpc.h says, without numpy's help."""
    T, B = word.shape
    out = {k: [[0] * G for _ in range(T)] for k in montecarlo.SERIES_INT_TABLES}
    out.update(e_sum=[[0.0] * G for _ in range(T)], e_max=[[math.nan] * G for _ in range(T)], e_q=[[[math.nan] * len(q) for _ in range(G)] for _ in range(T)])
    for t in range(T):
        for g in range(G):
            vals = []
            for b in range(B):
                w = int(word[t, b])
                if (0 if group is None else int(group[b])) != g or not w & 1:
                    continue
                out["n_alive"][t][g] += 1
                for i, k in enumerate(FLAGS):
                    out[k][t][g] += (w >> (i + 1)) & 1
                it, age = (w >> 8) & 4095, w >> 20
                out["iters_sum"][t][g] += it
                out["age_sum"][t][g] += age
                out["iters_max"][t][g] = max(out["iters_max"][t][g], it)
                out["age_max"][t][g] = max(out["age_max"][t][g], age)
                if math.isnan(e[t, b]):
                    out["n_nan"][t][g] += 1
                else:
                    vals.append(float(e[t, b]))
            vals.sort()
            if vals:
                out["e_max"][t][g] = vals[-1]
                out["e_q"][t][g] = [vals[int(math.floor(qq * (len(vals) - 1)))] for qq in q]
                out["e_sum"][t][g] = math.fsum(vals)
    return {k: np.array(v) for k, v in out.items()}


def _random_record(rng, T, B, G):
    group = rng.integers(-1, G, B)
    group[group == 2] = 3                                                      # group 2 is empty
    word = rng.integers(0, 2 ** 32, (T, B), dtype=np.uint64).astype(np.uint32) & np.uint32(0xffffff7f)
    word[1] &= np.uint32(0xfffffffe)                                           # a row with nobody alive
    e = np.round(rng.normal(size=(T, B)), 1)                                   # one decimal: many ties
    e[rng.uniform(size=(T, B)) < 0.1] = np.nan
    return e, word, group


def test_numpy_twin_against_a_python_loop():
    rng = np.random.default_rng(1)
    T, B, G = 4, 90, 5
    q = (0.0, 0.5, 0.95, 1.0, 0.3)
    e, word, group = _random_record(rng, T, B, G)
    one = np.flatnonzero((group == 4) & (word[3] & 1 == 1))                    # column (3, 4): exactly one value takes part
    word[3, one[1:]] &= np.uint32(0xfffffffe)
    e[3, one[0]] = -2.5
    for grp, ng in ((group, G), (None, 1)):
        got, want = montecarlo.series_stats(e, word, grp, q, G=ng), _naive_stats(e, word, grp, q, ng)
        for k in montecarlo.SERIES_INT_TABLES + ("e_max", "e_q"):
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k], equal_nan=True), k
        assert np.allclose(got["e_sum"], want["e_sum"], rtol=0, atol=1e-12)
        assert all(got[k].dtype == (np.int64 if k.endswith("_sum") else np.int32) for k in montecarlo.SERIES_INT_TABLES)
    got = montecarlo.series_stats(e, word, group, q, G=G)
    assert not got["n_alive"][1].any() and np.isnan(got["e_max"][1]).all() and np.isnan(got["e_q"][1]).all() and not got["e_sum"][1].any()
    assert not got["n_alive"][:, 2].any() and np.isnan(got["e_q"][:, 2]).all()                    # the empty group
    assert got["n_alive"][3, 4] == 1 and got["n_nan"][3, 4] == 0 and np.all(got["e_q"][3, 4] == -2.5) and got["e_max"][3, 4] == -2.5
    assert got["n_nan"].sum() > 0 and np.all(got["n_nan"] <= got["n_alive"])
    assert montecarlo.series_stats(e, word, group, (), G=G)["e_q"].shape == (T, G, 0)
    assert montecarlo.series_stats(e, word, group, q)["e_q"].shape == (T, G, len(q))              # G defaults to the largest id + 1


# ------------------------------------------------------------------------------------------------ 2: the host loops
def _lqr_packets(A, Bm, K, N, status_at=None, iters_at=None):
    """A stub controller: the LQR roll-out from the estimate as the packet, U_t[:, :, i] = -K (x_i - r), terminal column K r; status and
    iterations per call from the given functions of (call, batch)."""
    calls = []

    def packets(x_hat, r, g=None):
        nb = x_hat.shape[0]
        x, U = np.array(x_hat, dtype=np.float64), np.zeros((nb, Bm.shape[1], N + 1))
        for i in range(N):
            U[:, :, i] = -(x - r) @ K.T
            x = x @ A.T + U[:, :, i] @ Bm.T
        U[:, :, N] = r @ K.T
        t = len(calls)
        calls.append(1)
        st = np.zeros(nb, np.int32) if status_at is None else status_at(t, nb)
        it = np.full(nb, 5, np.int32) if iters_at is None else iters_at(t, nb)
        return U, np.array(x_hat), st, it
    return packets


def _host_setup(nb=24, T=30, seed=3):
    w = workloads.double_integrator()
    A, Bm = np.asarray(w["A"], dtype=np.float64), np.asarray(w["B"], dtype=np.float64)
    K = np.array([[0.5, 1.0]])
    th, ga, dist = montecarlo.draw_realisations(nb, T, w["w_bound"], seed=seed)
    rng = np.random.default_rng(seed)
    ch = dict(p_gb=rng.uniform(0.05, 0.5, nb), p_bg=rng.uniform(0.1, 0.9, nb), e_g=rng.uniform(0.0, 0.2, nb), e_b=rng.uniform(0.5, 1.0, nb))
    for k, v in zip(("p_gb", "p_bg", "e_g", "e_b"), (1.0, 0.0, 0.1, 1.0)):
        ch[k][1] = v                                                           # trajectory 1 loses every packet after step 0
    ref = np.where(np.arange(T) < T // 2, 2.0, -1.2)
    return A, Bm, K, th, ga, dist, ch, ref


def _check_identities(out, rows, N, tube_key="tube_violations", stopped=False):
    """The record of the trajectories `rows` against the loop's own sums and counters.  stopped: the trajectories ended at an infeasible
    solve, which not_optimal counts and the record -- written by the trajectories that TAKE a step -- does not."""
    s = out["series"]
    T = s["e"].shape[0]
    acc = np.zeros(s["e"].shape[1])
    for t in range(T):
        acc += s["e"][t]                                                       # the loop's order: step by step
    assert acc[rows].tobytes() == np.asarray(out["err2"])[rows].tobytes()
    for key, flag in (("lost_up", "lost_up"), ("lost_down", "lost_down"), ("overrun", "overrun"), (tube_key, "tube"), ("not_optimal", "not_optimal")):
        if key in out:
            assert np.array_equal(s[flag].sum(axis=0)[rows] + (1 if stopped and key == "not_optimal" else 0), np.asarray(out[key])[rows]), key
    assert np.array_equal(s["age"].max(axis=0)[rows], out["max_gap"][rows])
    assert np.array_equal(s["overrun"], s["alive"] & (s["age"] >= N))
    assert np.array_equal(montecarlo.pack_series_word(**{k: s[k] for k in ("alive",) + FLAGS + ("iters", "age")}), s["word"])


@pytest.mark.parametrize("full_ref", [False, True])
@pytest.mark.parametrize("extended", [False, True])
def test_tube_host_loop_record_adds_up_to_its_statistics(extended, full_ref):
    N = 4
    A, Bm, K, th, ga, dist, ch, ref = _host_setup()
    nb, T = th.shape
    Z = Polytope(np.r_[np.eye(2), -np.eye(2)], 0.05 * np.ones(4))              # a tight tube: some steps leave it
    status = lambda t, n: ((np.arange(n) + t) % 7 == 0).astype(np.int32)       # some solves "not optimal" (status 1)
    iters = lambda t, n: ((np.arange(n) * 37 + t * 11) % 60).astype(np.int32)
    if full_ref:
        ref = np.stack([np.tile(ref[None], (nb, 1)), 0.1 * np.ones((nb, T))], axis=2)
    kw = dict(extended=extended, channel=ch)
    plain = montecarlo.run_remote_tube_mpc(_lqr_packets(A, Bm, K, N, status, iters), A, Bm, K, K, N, Z, None, ref, th, ga, dist, **kw)
    out = montecarlo.run_remote_tube_mpc(_lqr_packets(A, Bm, K, N, status, iters), A, Bm, K, K, N, Z, None, ref, th, ga, dist, series=True, **kw)
    assert "series" not in plain
    for k in ("tracking_error", "tube_violations", "not_optimal", "x_final", "lost_up", "lost_down", "max_gap", "overrun"):
        assert np.array_equal(plain[k], out[k]), k                            # recording changes nothing
    s = out["series"]
    assert s["e"].shape == s["word"].shape == (T, nb) and s["alive"].all()
    _check_identities(out, np.arange(nb), N)
    assert np.array_equal(out["tracking_error"], np.sqrt(out["err2"]) / T)
    assert np.array_equal(s["iters"], np.array([iters(t, nb) for t in range(T)]))
    assert out["tube_violations"].sum() > 0 and out["not_optimal"].sum() > 0 and out["overrun"][1] == T - N and s["age"][:, 1].tolist() == list(range(T))
    assert s["adopted"][0].all() and not s["adopted"][1:, 1].any() and not s["lost_up"][0].any()


def test_rmpc_host_loop_record_stops_with_the_trajectory():
    N = 4
    A, Bm, K, th, ga, dist, ch, ref = _host_setup(seed=4)
    nb, T = th.shape
    stop = {3: 0, 7: 11, 12: T - 1}                                            # trajectory: the step of its infeasible solve

    def status(t, n):
        st = ((np.arange(n) + t) % 9 == 0).astype(np.int32)
        for b, at in stop.items():
            if t == at:
                st[b] = 2
        return st
    out = montecarlo.run_remote_tracking_mpc(_lqr_packets(A, Bm, K, N, status), A, Bm, K, N, None, ref, th, ga, dist, channel=ch, series=True)
    s = out["series"]
    dead = out["infeasible"]
    assert sorted(np.flatnonzero(dead)) == sorted(stop) and np.isnan(out["tracking_error"][dead]).all()
    for b, at in stop.items():
        assert s["alive"][:at, b].all() and not s["word"][at:, b].any() and not s["e"][at:, b].any()
    live = np.flatnonzero(~dead)
    assert s["alive"][:, live].all()
    _check_identities(out, live, N)
    _check_identities(out, np.flatnonzero(dead), N, stopped=True)              # and what a stopped trajectory counted up to its stop
    assert not s["tube"].any()


def test_sweep_refuses_a_sharded_series():
    with pytest.raises(ValueError, match="series needs world == 1"):
        montecarlo.mc_sweep(None, dict(w_bound=np.zeros(2)), [0.0, 0.5], 2, 5, 0.5, world=2, series=True)


# ------------------------------------------------------------------------------------------------ 3: the refusals
@pytest.fixture(scope="module")
def host_handle(hip_lib):
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True, device=-1)
    yield mpc._handle
    mpc._close()


def test_exports_exist_and_are_bound(hip_lib):
    L = _native.lib()
    for name, nargs in (("tmpc_mc_set_series", 2), ("tmpc_mc_get_series", 5), ("tmpc_mc_series_stats", 23), ("tmpc_series_stats", 25)):
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == nargs, name
    for name in ("mc_get_series", "mc_series_stats", "series_stats"):
        assert callable(getattr(_native, name))
    assert _native.ABI_VERSION == L.tmpc_abi_version() == 5                    # added without a bump
    assert L.tmpc_mc_set_series(None, 1) == E_INVALID and L.tmpc_mc_get_series(None, 1, 1, None, None) == E_INVALID


def _raw_stats(B, T, G, e=True, word=True, group=None, n_q=0, q=None, device=-1):
    keep = []

    def arr(v, dtype, n):
        if v is None:
            return None
        a = np.zeros(max(n, 1), dtype) if v is True else np.ascontiguousarray(v, dtype=dtype)
        keep.append(a)
        return a.ctypes.data
    n = max(B, 1) * max(T, 1)
    rc = _native.lib().tmpc_series_stats(device, B, T, arr(e, np.float64, n), arr(word, np.uint32, n), G, arr(group, np.int32, B), n_q,
                                         arr(q, np.float64, n_q), *[None] * 16)
    return rc, _native.lib().tmpc_last_error(None).decode()


def test_series_stats_finds_every_argument_error_before_the_device():
    ok_q = [0.0, 0.5, 1.0]
    for kw, name in ((dict(B=0), "B < 1"), (dict(T=0), "T < 1"), (dict(G=0), "G < 1"), (dict(B=-3), "B < 1"), (dict(e=None), "e is NULL"),
                     (dict(word=None), "word is NULL"), (dict(group=[0, 1, 2, 0]), "group[2] = 2"), (dict(group=[0, -2, 1, 0]), "group[1] = -2"),
                     (dict(n_q=-1), "n_q = -1"), (dict(n_q=17, q=np.zeros(17)), "n_q = 17"), (dict(n_q=3, q=None), "q is NULL"),
                     (dict(n_q=3, q=[0.0, 1.5, 1.0]), "q[1] = 1.5"), (dict(n_q=3, q=[-0.1, 0.5, 1.0]), "q[0] = -0.1"),
                     (dict(n_q=3, q=[0.0, 0.5, np.nan]), "q[2] = nan")):
        args = dict(B=4, T=3, G=2, n_q=0)
        args.update(kw)
        rc, msg = _raw_stats(**args)
        assert rc == E_INVALID and msg.startswith("tmpc_series_stats: ") and name in msg, (kw, rc, msg)
    # sound arguments: only the device is missing
    rc, msg = _raw_stats(4, 3, 2, group=[0, 1, -1, 0], n_q=3, q=ok_q)
    assert rc == E_DEVICE and "device < 0" in msg
    rc, msg = _raw_stats(4, 3, 2, n_q=16, q=np.linspace(0, 1, 16))
    assert rc == E_DEVICE
    with pytest.raises(RuntimeError, match=r"tmpc_series_stats failed \(-1\).*q\[0\] = 2"):
        _native.series_stats(np.zeros((3, 4)), np.zeros((3, 4), np.uint32), q=(2.0,), device=-1)
    with pytest.raises(ValueError, match="group holds 3 entries"):
        _native.series_stats(np.zeros((3, 4)), np.zeros((3, 4), np.uint32), group=[0, 0, 0], device=-1)


def test_setter_and_getters_on_host_only_handles(host_handle):
    h, L = host_handle, _native.lib()
    e, w = np.zeros((5, 3)), np.zeros((5, 3), np.uint32)
    assert L.tmpc_mc_get_series(h.ptr, 3, 5, e.ctypes.data, w.ctypes.data) == E_INVALID and "tmpc_mc_get_series" in h.error()      # nothing has run
    assert L.tmpc_mc_set_series(h.ptr, 1) == 0                                                     # works without a device
    try:
        assert L.tmpc_mc_get_series(h.ptr, 3, 5, e.ctypes.data, w.ctypes.data) == E_INVALID        # still nothing has run
        q = np.array([0.5])
        args = [None] * 16
        assert L.tmpc_mc_series_stats(h.ptr, 3, 5, 1, None, 1, q.ctypes.data, *args) == E_INVALID and "tmpc_mc_set_series" in h.error()
        grp = np.array([0, 1, 0], np.int32)
        assert L.tmpc_mc_series_stats(h.ptr, 3, 5, 1, grp.ctypes.data, 1, q.ctypes.data, *args) == E_INVALID and "group[1] = 1" in h.error()
        assert L.tmpc_mc_series_stats(h.ptr, 3, 5, 1, None, 17, q.ctypes.data, *args) == E_INVALID and "n_q = 17" in h.error()
        # a recording loop on a host-only handle ends where every loop does there
        with pytest.raises(RuntimeError, match="host-only"):
            _native.mc_run(h, np.zeros(3), np.zeros(5), np.zeros((3, 5)), np.zeros((3, 5)), np.zeros((3, 5, h.nx)), series=True)
        with pytest.raises(RuntimeError, match="per-step record"):
            _native.mc_series_stats(h)
    finally:
        assert L.tmpc_mc_set_series(h.ptr, 0) == 0
    reg = rp.plain_double_integrator(device=-1)
    try:
        hr = reg._handle if hasattr(reg, "_handle") else reg
        assert L.tmpc_mc_set_series(hr.ptr, 1) == E_INVALID and "regulator" in hr.error()
    finally:
        if hasattr(reg, "_close"):
            reg._close()


# ------------------------------------------------------------------------------------------------ 4: the kernel's source on the host model
@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    """The host-model programs under the sanitizers (tests/wavesim/hostsim.py: a host without their runtimes skips, a program that does not
    build fails).  Stand-alone programs: nothing is loaded into Python under a sanitizer."""
    return hostsim.binaries_or_skip(tmp_path_factory, "seriessim")


def _assert_equals_twin(out, e, word, group, q, G):
    ref = montecarlo.series_stats(e, word, group, q, G=G)
    for k in series_case.EXACT:
        assert out[k].dtype == ref[k].dtype and out[k].tobytes() == ref[k].tobytes(), k
    bound = series_case.e_sum_bound(e, word, np.zeros(word.shape[1], np.int32) if group is None else group, G)
    fin = np.isfinite(bound)
    gap = np.abs(out["e_sum"][fin] - ref["e_sum"][fin])
    assert np.all(gap <= bound[fin]), float(np.max(gap - bound[fin]))
    assert np.array_equal(out["e_sum"][~fin], ref["e_sum"][~fin])              # a column with +inf sums to +inf in any order
    return ref


@pytest.mark.parametrize("build", ["seriessim_asan", "seriessim_msan"])
def test_reduction_kernel_on_the_host_model(binaries, build):
    """The edge record of the GPU test at its full size (3 steps, groups of 0 .. 2049 interleaved, -1 members, a group of dead words), all
    sixteen quantiles' worth of LDS in use, and the same record as one group of everybody without quantiles."""
    e, word, group, G = series_case.edge_record()
    q16 = series_case.QUANTILES + tuple(np.linspace(0.01, 0.99, 11))
    for grp, ng, q in ((group, G, q16), (None, 1, ()), (group, G, series_case.QUANTILES[:1])):
        out = series_case.run_stats(binaries[build], e, word, grp, q, ng, env=hostsim.SAN_ENV)
        hostsim.assert_clean(out["stderr"])
        ref = _assert_equals_twin(out, e, word, grp, q, ng)
    assert ref["n_alive"][0].tolist() == list(series_case.SIZES) + [0] and np.isnan(ref["e_q"][:, [0, G - 1]]).all()
