"""The closed loops through the explicit law, without a GPU: the refusals of the new C entry points (include/tmpc.h: tmpc_mc_set_law,
tmpc_mc_get_law_stats, tmpc_mc_get_law_misses) on host-only handles, the host twin of the law loop (montecarlo.LawPackets) against the
oracle-driven host loop with a table learnt through the numpy twin (explicit_law.region_law / locate), and the resource notes of the fused
kernel's code objects.  The loops themselves run in tests/test_law_loop_gpu.py.

Bounds.  A hit's first input against the oracle's: TOL_U0 = 1e-8 of tests/certificates.py.  The twin's loop against the oracle's loop: the
bounds tests/test_closed_loop.py gives the device solver against the oracle in the same loop (x_final 1e-7, tracking_error 1e-9)."""
import importlib.util
import os

import numpy as np
import pytest

import common
from LinearMPCOverNetworks import explicit_law as E
from LinearMPCOverNetworks import montecarlo
from LinearMPCOverNetworks import sensitivity as S
from oracle.oracle import Oracle

ROOT = os.path.dirname(common.PKG)
TOL_U0 = 1e-8                             # tests/certificates.py
E_INVALID, E_UNSUPPORTED = -1, -2


# ------------------------------------------------------------------ refusals
def test_setter_and_getters_on_host_only_handles(hip_lib):
    import regulator_problems
    L = hip_lib.lib()
    plain, _ = common.make_mpc("cartpole", 10, True, create=True, device=-1)
    reg = regulator_problems.plain_double_integrator(device=-1)
    try:
        h = plain._handle
        hits, tries, region = np.zeros(4, np.int32), np.zeros(4, np.int64), np.zeros(4, np.int32)
        n_total = np.zeros(1, np.int64)
        # the getters before any run
        assert L.tmpc_mc_get_law_stats(h.ptr, 4, hits.ctypes.data, tries.ctypes.data, region.ctypes.data) == E_INVALID
        assert "no tracking loop of this B has run through the explicit law" in h.error()
        assert L.tmpc_mc_get_law_misses(h.ptr, 4, n_total.ctypes.data, None, None, None) == E_INVALID
        assert "tmpc_mc_get_law_misses" in h.error()
        # the setter stores the setting on a host-only handle; a negative capacity is refused and changes nothing
        assert L.tmpc_mc_set_law(h.ptr, 1, 4, 16) == 0
        assert L.tmpc_mc_set_law(h.ptr, 1, 0, -1) == E_INVALID and h.error() == "tmpc_mc_set_law: miss_capacity < 0"
        assert L.tmpc_mc_set_law(h.ptr, 1, -3, 0) == 0          # (max_tries <= 0: all)
        assert L.tmpc_mc_set_law(h.ptr, 0, 0, 0) == 0
        # still no loop: the getters stay refused, with any B, a NULL handle and a negative capacity too
        assert L.tmpc_mc_get_law_stats(h.ptr, 0, None, None, None) == E_INVALID
        assert L.tmpc_mc_get_law_misses(h.ptr, -1, None, None, None, None) == E_INVALID and "capacity < 0" in h.error()
        assert L.tmpc_mc_set_law(None, 1, 0, 0) == E_INVALID and L.tmpc_mc_get_law_stats(None, 1, None, None, None) == E_INVALID
        assert L.tmpc_mc_get_law_misses(None, 1, None, None, None, None) == E_INVALID
        # a regulator handle
        r = reg._handle
        assert L.tmpc_mc_set_law(r.ptr, 1, 0, 0) == E_UNSUPPORTED and "regulator handle" in r.error()
        assert L.tmpc_mc_set_law(r.ptr, 0, 0, 0) == E_UNSUPPORTED
        assert L.tmpc_mc_get_law_stats(r.ptr, 1, None, None, None) == E_INVALID
    finally:
        plain._close()
        reg._close()


def test_law_setting_forms(hip_lib):
    assert hip_lib._law_setting(None) == (0, 0, 0) and hip_lib._law_setting(False) == (0, 0, 0) and hip_lib._law_setting(True) == (1, 0, 0)
    assert hip_lib._law_setting(4) == (1, 4, 0) and hip_lib._law_setting(dict(max_tries=2, miss_capacity=9)) == (1, 2, 9)
    assert hip_lib._law_setting(dict(miss_capacity=3)) == (1, 0, 3)
    with pytest.raises(ValueError, match="unknown keys"):
        hip_lib._law_setting(dict(capacity=3))


# ------------------------------------------------------------------ the host twin against the oracle-driven loop
def _oracle_packets(mpc, orc):
    def fn(x_hat, r, gamma=None):
        sol = orc.solve(x_hat, r, gamma)
        u_ss = sol["u_ss"] + sol["x_ss"] @ mpc._K.T
        U = np.concatenate([sol["u_nom"], u_ss[:, None, :]], axis=1).transpose(0, 2, 1)
        return np.ascontiguousarray(U), sol["x_nom0"], sol["status"]
    return fn


def scenario(w, B, T, seed=61, amp=0.5):
    """The scenario of tests/test_law_loop_gpu.py (its _scenario)."""
    th, ga, dist = montecarlo.draw_realisations(B, T, w["w_bound"], seed=seed)
    return dict(p_loss=(np.arange(B) % 4) * 0.3, ref=np.where(np.arange(T) < (T + 1) // 2, amp, -0.6 * amp), th_u=th, ga_u=ga, w=dist)


def test_host_twin_against_the_oracle_loop(oracle_lib, hip_lib):
    """A pilot through an empty table logs every state; their working sets (the numpy twin of the sensitivity kernel on the oracle's solutions)
    become the table; the second sweep hits, and a hit's packet is the oracle's.  This is the scenario of the GPU tests at B = 12: the
    share of hits they rely on (at least half of the steps) is confirmed here."""
    B, T, N = 12, 12, 10
    mpc, w = common.make_mpc("cartpole", N, True, create=True, device=-1)
    try:
        orc = Oracle(mpc._problem_dict())
        K, Kp = mpc.get_steady_state_controller_gain(), mpc.get_ancillary_controller_gain()
        sc = scenario(w, B, T)
        fn = _oracle_packets(mpc, orc)

        def loop(packets):
            return montecarlo.run_remote_tube_mpc(packets, w["A"], w["B"], K, Kp, N, mpc._Z, sc["p_loss"], sc["ref"], sc["th_u"], sc["ga_u"], sc["w"])
        solved = loop(fn)
        pilot = montecarlo.LawPackets.from_tables(fn, [], K, N, miss_capacity=B * T)
        first = loop(pilot)
        log = pilot.result()["misses"]
        assert pilot.steps == B * T and log["n_total"] == B * T and len(log["x_k"]) == B * T and np.all(pilot.hits == 0) and np.all(pilot.tries == 0)
        for k in ("x_final", "err2", "tube_violations", "not_optimal", "lost_up", "lost_down", "max_gap", "overrun"):
            assert np.array_equal(first[k], solved[k]), k               # an empty table is the solved loop
        # the table: the distinct working sets of the logged states
        sol = orc.solve(log["x_k"], log["ref"])
        tw = S.handle_sensitivity(mpc, log["x_k"], log["ref"], {k: sol[k] for k in ("u_nom", "x_nom0", "xu_ss", "status")})
        ok = (tw["flag"] & (S.SKIPPED | S.NOT_KKT)) == 0
        model = E.law_model(mpc._handle, 0)
        nc = model["G"].shape[0]
        sets = []
        for a in tw["active"][ok]:
            rows = tuple(S.decode_active(a[:(nc + 31) // 32], nc=nc))
            if rows not in sets:
                sets.append(rows)
        table = [E.region_law(model, s) for s in sets]
        assert len(table) >= 2 and all(t is not None for t in table)
        # the second sweep
        seen = []

        def checked(x_hat, r):
            seen.append((x_hat.copy(), r.copy()))
            return fn(x_hat, r)
        for max_tries in (0, 1):
            twin = montecarlo.LawPackets.from_tables(checked, table, K, N, max_tries=max_tries, miss_capacity=5)
            # a hit gives the oracle's first input
            x_probe, r_probe = log["x_k"][ok], log["ref"][ok]
            U, x0, st, it = twin(x_probe, r_probe)
            hit = twin.region >= 0
            want = orc.solve(x_probe, r_probe)
            assert hit.all() or max_tries == 1
            assert np.all(st[hit] == 0) and np.all(it[hit] == 0)
            assert np.max(np.abs(U[hit][:, :, 0] - want["u_nom"][hit][:, 0, :])) <= TOL_U0
            assert np.max(np.abs(x0[hit] - want["x_nom0"][hit])) <= TOL_U0
            twin = montecarlo.LawPackets.from_tables(checked, table, K, N, max_tries=max_tries, miss_capacity=5)
            second = loop(twin)
            res = twin.result()
            n_hits, n_miss = int(res["law_hits"].sum()), res["misses"]["n_total"]
            print(f"max_tries {max_tries}: {len(table)} regions, {n_hits} of {B * T} steps hit, mean tries {res['law_tries'].sum() / (B * T):.2f}")
            assert n_hits + n_miss == B * T == twin.steps                   # hits + misses = steps taken
            assert len(res["misses"]["x_k"]) == min(5, n_miss)
            assert sum(twin.region_hits[0].values()) == n_hits
            if max_tries == 0:
                assert n_hits >= B * T // 2                                 # the condition the GPU tests rely on
                assert np.all(res["law_tries"] >= res["law_hits"])
            np.testing.assert_allclose(second["x_final"], solved["x_final"], atol=1e-7, rtol=0)
            np.testing.assert_allclose(second["tracking_error"], solved["tracking_error"], atol=1e-9, rtol=0)
            for k in ("not_optimal", "lost_up", "lost_down", "max_gap", "overrun"):
                assert np.array_equal(second[k], solved[k]), k
    finally:
        mpc._close()


# ------------------------------------------------------------------ the fused kernel's code objects
def test_fused_law_kernels_keep_the_register_budget(hip_lib):
    """closed_loop_law<shape> is solve_kernel<shape>'s body behind the law's walk: no scratch, at most 24 registers over its twin (the rule
    tests/test_code_objects.py applies to closed_loop_kernel), the bench shape within the 256 registers of two waves per SIMD without a
    spill.  The dense-single shapes are left out of csrc/tmpc_fused_law.hip (they would need 28 - 29 over their twins): their handles look
    the law up per time step."""
    spec = importlib.util.spec_from_file_location("code_object_notes", os.path.join(ROOT, "scripts", "code_object_notes.py"))
    notes = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(notes)
    ks = notes.kernels(os.path.join(common.PKG, "lib", "libtmpc_hip.so"))
    dm = notes.demangle(list(ks))
    ks = {dm[n]: k for n, k in ks.items()}
    fused = {n: k for n, k in ks.items() if "::closed_loop_law<" in n}
    wave = {n.split("::solve_kernel")[1].split("(")[0]: k for n, k in ks.items() if "::solve_kernel<" in n}
    assert len(fused) == 7, sorted(fused)
    for n, k in fused.items():
        # none of the name filters of the existing tests catches it
        assert not any(f in n for f in ("::solve_kernel<", "::closed_loop_kernel<", "::closed_loop_step_kernel<", "law_kernel")), n
        shape = n.split("::closed_loop_law")[1].split("(")[0]
        assert int(shape.strip("<>").split(",")[3]) > 0, n                  # a factored block
        twin = wave[shape]
        assert k[".vgpr_count"] <= twin[".vgpr_count"] + 24, (n, k[".vgpr_count"], twin[".vgpr_count"])
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
    bench = [k for n, k in fused.items() if "closed_loop_law<11, 1, 0, 5, 4, 0, 8>" in n]
    assert len(bench) == 1 and bench[0][".vgpr_count"] <= 256 and bench[0][".vgpr_spill_count"] == 0 and bench[0][".private_segment_fixed_size"] == 0


# ------------------------------------------------------------------ the fused kernel's source on the host execution model
@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    """The host-model programs under the sanitizers (tests/wavesim/hostsim.py: a host without their runtimes skips, a program that does not
    build fails).  Stand-alone programs: nothing is loaded into Python under a sanitizer."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "wavesim"))
    import hostsim
    import law_loop_case
    return law_loop_case, hostsim.binaries_or_skip(tmp_path_factory, "lawloop")


@pytest.fixture(scope="module")
def sim_tables(oracle_lib, hip_lib):
    """The bench problem, its oracle, and the three tables: empty; three regions of which the second is the region of the first step's state
    (the first holds no p, the third is the region of a golden state); one region, that of the first step's state with its LAST row made to
    fail -- the candidate passes every chunk but the last."""
    mpc, w = common.make_mpc("cartpole", 10, True, create=True, device=-1)
    orc = Oracle(mpc._problem_dict())
    model = E.law_model(mpc._handle, 0)
    nc = model["G"].shape[0]
    G = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
    X = np.r_[np.zeros((1, 4)), G[7:8, :4]]
    R = np.r_[np.array([[0.5, 0.0, 0.0, 0.0]]), G[7:8, 4:]]
    sol = orc.solve(X, R)
    tw = S.handle_sensitivity(mpc, X, R, {k: sol[k] for k in ("u_nom", "x_nom0", "xu_ss", "status")})
    assert np.all((tw["flag"] & (S.SKIPPED | S.NOT_KKT)) == 0)
    regs = [E.region_law(model, S.decode_active(a[:(nc + 31) // 32], nc=nc)) for a in tw["active"]]
    assert all(r is not None for r in regs)
    last = {k: v.copy() for k, v in regs[0].items()}
    last["s"][-1] = -1e3
    nrow = len(regs[0]["s"])
    assert (nrow - 1) // 64 == ((nrow + 63) // 64 * 64 - 1) // 64 and nrow > 64          # (the last row lies in the last of several chunks)
    shape = (regs[0]["Ky"].shape[1], regs[0]["Ky"].shape[0], nrow)
    yield mpc, w, orc, shape, {"empty": [], "three": [None, regs[0], regs[1]], "last_chunk": [last]}
    mpc._close()


@pytest.mark.parametrize("build", ["lawloop_asan", "lawloop_msan"])
@pytest.mark.parametrize("which", ["empty", "three", "last_chunk"])
def test_fused_kernel_source_on_the_host_model(binaries, sim_tables, build, which):
    """csrc/tmpc_kernels.hip with FUSED = 3 compiled for the CPU under ASan + UBSan and under MSan (bench shape, B in {1, 9}, T = 3): region,
    tries, hits, the per-region counters and the miss log equal the host twin's (montecarlo.LawPackets on the same tables, the oracle behind
    it); the logged states, which two solvers produced, to TOL_U0."""
    import hostsim
    law_loop_case, bins = binaries
    mpc, w, orc, shape, tables = sim_tables
    table = tables[which]
    T, N = 3, 10
    K, Kp = mpc.get_steady_state_controller_gain(), mpc.get_ancillary_controller_gain()
    for B in (1, 9):
        sc = scenario(w, B, T)
        for max_tries in ((0, 1) if which == "three" else (0,)):
            twin = montecarlo.LawPackets.from_tables(_oracle_packets(mpc, orc), table, K, N, max_tries=max_tries, miss_capacity=B * T - 1)
            host = montecarlo.run_remote_tube_mpc(twin, w["A"], w["B"], K, Kp, N, mpc._Z, sc["p_loss"], sc["ref"], sc["th_u"], sc["ga_u"], sc["w"])
            res = twin.result()
            out = law_loop_case.run(bins[build], mpc._problem_dict(), K, Kp, mpc._Z, sc["p_loss"], sc["ref"], sc["th_u"], sc["ga_u"], sc["w"], table, shape,
                                    max_tries=max_tries, miss_capacity=B * T - 1, warm=(B == 9), env=hostsim.SAN_ENV)
            hostsim.assert_clean(out["stderr"])
            assert np.array_equal(out["region"], res["law_region"]) and np.array_equal(out["hits"], res["law_hits"]), (which, B, max_tries)
            assert np.array_equal(out["tries"], res["law_tries"]), (which, B, max_tries, out["tries"], res["law_tries"])
            want = np.array([twin.region_hits[0].get(r, 0) for r in range(len(table))], np.uint64)
            assert np.array_equal(out["region_hits"], want)
            log = res["misses"]
            assert out["n_total"] == log["n_total"] and int(out["hits"].sum()) + out["n_total"] == B * T
            assert len(out["x_k"]) == len(log["x_k"]) == min(log["n_total"], B * T - 1) and np.all(out["variant"] == 0)
            if which == "three" and max_tries == 0:
                assert out["hits"].sum() >= B                                  # (the first step's state at least)
            else:
                assert which == "three" or (out["hits"].sum() == 0 and np.all(out["tries"] == T * len(table)))
            # the one-workgroup model runs its waves in turn, and so does the twin: the rows come in the same order unless a trajectory dies (none does)
            key = lambda m: np.c_[m["x_k"], m["ref"]][np.lexsort(np.round(np.c_[m["x_k"], m["ref"]], 6).T[::-1])]
            if len(log["x_k"]) == log["n_total"]:
                assert np.max(np.abs(key(out) - key(log)), initial=0.0) <= TOL_U0
            np.testing.assert_allclose(out["x_final"], host["x_final"], atol=1e-7, rtol=0)
            assert np.array_equal(out["not_optimal"], host["not_optimal"]) and np.array_equal(out["tube_violations"], host["tube_violations"])
