"""The hops of the explicit law's search on the GPU (include/tmpc.h: tmpc_law_set_hops, tmpc_qp_law_eval_hops; csrc/tmpc_law_wave.hpp).

Exact: region, tries and the chains' six counters against the numpy twin (explicit_law.locate, montecarlo.LawPackets); max_hops = 0
against the entries without hops, the one-launch loop against the per-step loop, an empty table against the law off, all by bytes.
At a tolerance: y of the clipped family against the closed form, 1e-11 max|y| (tests/test_explicit_law_gpu.py's bound); a loop through the
table against the solved loop at the bounds tests/test_closed_loop.py gives warm against cold (x_final 1e-8, tracking_error 1e-10)."""
import os
import runpy
import sys

import numpy as np
import pytest

import certificates
import common
import law_cases as lc
import law_hop_cases as hc
from LinearMPCOverNetworks import explicit_law as E
from LinearMPCOverNetworks import montecarlo
from test_law_loop_gpu import KEYS, LAW_KEYS, _close_to, _learn, _rows, _run, _same, _scenario, _stepped

pytestmark = pytest.mark.gpu

STATES = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
OUT = ("u_nom", "x_nom0", "xu_ss", "x_nom", "status", "iters")
HITS, TESTS, ABSENT, CAP, CYCLE, PAR = range(6)

# ------------------------------------------------------------------ 1: the clipped family through tmpc_qp_law_eval_hops
def _table(c, nv, nc, npar):
    """The table of a case (tests/law_hop_cases.py: hop_table): whole paths from a common start -- the first instance's own set without its
    first rows -- for as many instances as the cap allows, of the others the first hop and their own set (their chains end at an absent
    neighbour and the walk answers), and decoys.  Where a region is wide (nc = 2049: building one costs tens of milliseconds on the host) few
    paths, few decoys, and the other instances may miss."""
    wide = nc > 1000
    return hc.hop_table(c, c["sets"][0][3:], 12 if wide else 40 if nv > 17 and npar > 8 else 120, decoys=8 if wide else 32, seed=npar, keep_rest=not wide)


@pytest.mark.parametrize("nc", [1, 63, 64, 65, 2049])
@pytest.mark.parametrize("nv", [1, 17, 128])
def test_clipped_family_with_hops(hip_lib, nv, nc):
    calls = chain_hits = 0
    for npar in (1, 8, 32):
        # one case of 65 instances and its table per (nv, nc, np); the batches are its first B instances
        c = lc.clipped_case(1000 + 7 * nv + nc + npar, nv, nc, npar, 65)
        m = c["model"]
        sets, start, full = _table(c, nv, nc, npar)
        table = [E.region_law(m, s) for s in sets]
        assert all(t is not None for t in table) and full[0]
        R = len(sets)
        words = np.array([E.words_of(s, nc) for s in sets], dtype=np.uint32).reshape(R, (nc + 31) // 32)
        ymax = max(1.0, float(np.abs(c["Z"]).max()))
        for B in (1, 63, 65):
            P, Z = c["P"][:B], c["Z"][:B]
            order = np.random.default_rng(B).permutation(R).astype(np.int32)
            hint = np.array([(start, -1, R + 5)[b % 3] for b in range(B)], np.int32)
            args = (m["H"], m["F"], m["G"], m["g0"], m["Ebar"], m["Y"], m["Yp"], words, order, P)
            for mt in (0, 2):
                plain = hip_lib.qp_law_eval(*args, hint=hint, max_tries=mt)
                for mh in (0, 1, 200):
                    dev = hip_lib.qp_law_eval(*args, hint=hint, max_tries=mt, max_hops=mh, want_stats=True)
                    st = np.zeros(6, np.int64)
                    region, tries, _ = E.locate(table, P, hint=hint, order=order, max_tries=mt, max_hops=mh, nc=nc, stats=st)
                    case = (nv, nc, npar, B, mt, mh)
                    assert np.array_equal(dev["region"], region) and np.array_equal(dev["tries"], tries), case
                    assert np.array_equal(dev["stats"], st), (case, dev["stats"], st)
                    hit = region >= 0
                    assert np.all(np.isnan(dev["y"][~hit]))
                    assert np.max(np.abs(dev["y"][hit] - Z[hit]), initial=0.0) <= 1e-11 * ymax, case
                    if mh == 0:
                        assert all(dev[k].tobytes() == plain[k].tobytes() for k in ("y", "region", "tries")) and not st.any()
                    if mh == 200 and mt == 0:
                        assert hit.all() or nc > 1000                # (the wide tables hold whole paths only)
                        for b in range(B):
                            if hint[b] == start and full[b]:
                                assert hit[b] and tries[b] == 1 + hc.dist(c, sets[start], b), (case, b)
                        assert st[HITS] >= sum(1 for b in range(B) if hint[b] == start and full[b]) >= 1
                        chain_hits += int(st[HITS])
                    calls += 1
    assert calls == 54 and chain_hits >= 9


# ------------------------------------------------------------------ 2: cart-pole handles
def _bytes(out, keys=OUT + ("region", "tries")):
    return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in keys)


@pytest.mark.parametrize("which", ["fixed", "free", "extended"])
def test_cartpole_handles_with_hops(hip_lib, which):
    import torch
    B = 256
    X, R = np.ascontiguousarray(STATES[:B, :4]), np.ascontiguousarray(STATES[:B, 4:])
    mpc, _ = common.make_mpc("cartpole", 10, which != "free", extended=which == "extended", create=True)
    var = None if which != "extended" else (np.arange(B) % 2).astype(np.uint8)
    try:
        h = mpc._handle
        law = mpc.explicit_law()
        plain = mpc._solve(X, R, variant=var)
        ids, n_new = hip_lib.law_learn(h, X, R, plain, variant=var)
        assert n_new >= 8
        off = hip_lib.law_eval(h, X, R, variant=var)
        assert not any(hip_lib.law_hop_stats(h, k).any() for k in range(h.nvariants))          # hops off: the counters are not touched
        # the hint of state b: the region of state b - 1 (of the same problem)
        step = 1 if var is None else 2
        hint = np.r_[np.full(step, -1), off["region"][:-step]].astype(np.int32)
        off_h = hip_lib.law_eval(h, X, R, variant=var, hint=hint)
        law.set_hops(64)
        assert law.max_hops == 64
        on = hip_lib.law_eval(h, X, R, variant=var, hint=hint)
        st = sum(hip_lib.law_hop_stats(h, k) for k in range(h.nvariants))
        assert np.array_equal(on["region"] >= 0, off["region"] >= 0)
        hit = on["region"] >= 0
        # a region that accepts gives the minimiser: where the two searches found different regions the outputs still agree
        assert np.max(np.abs(on["u_nom"][hit] - off["u_nom"][hit])) <= 2 * certificates.TOL_U0
        # (with hops on an unhinted instance chains from order[0]: every instance has a chain)
        assert st[HITS] + st[ABSENT] + st[CAP] + st[CYCLE] + st[PAR] <= B
        assert st[TESTS] <= on["tries"].sum() and st[TESTS] >= B and st[HITS] >= 1
        print(f"{which}: {n_new} regions, {int(hit.sum())} of {B} hit; the chain found {st[HITS]} ({st[HITS] / max(1, hit.sum()):.0%}) in {st[TESTS]} tests; ended "
              f"absent {st[ABSENT]}, cap {st[CAP]}, cycle {st[CYCLE]}, parameter row {st[PAR]}; mean tries {on['tries'].mean():.1f} with hops, "
              f"{off_h['tries'].mean():.1f} with the hint alone")
        sv = hip_lib.law_solve(h, X, R, variant=var, hint=hint)
        assert np.array_equal(sv["region"], on["region"]) and np.array_equal(sv["tries"], on["tries"])
        assert np.all((sv["status"] == 0) | (sv["status"] == 2)) and np.all(sv["iters"][hit] == 0)
        cert = certificates.certify_outputs(mpc, X, R, sv, variant=var)
        assert cert["n_opt"] >= 128
        # the device entries: the same bytes
        t = dict(x=torch.from_numpy(X).cuda(), r=torch.from_numpy(R).cuda(), hint=torch.from_numpy(hint).cuda(),
                 var=None if var is None else torch.from_numpy(var).cuda())
        N, nu = h.N, h.nu
        for name, host in (("law_eval_device", on), ("law_solve_device", sv)):
            o = dict(u_nom=torch.empty((B, N, nu), dtype=torch.float64, device="cuda"), x_nom0=torch.empty((B, 4), dtype=torch.float64, device="cuda"),
                     xu_ss=torch.empty((B, 4 + nu), dtype=torch.float64, device="cuda"), x_nom=torch.empty((B, N + 1, 4), dtype=torch.float64, device="cuda"),
                     status=torch.empty(B, dtype=torch.int32, device="cuda"), iters=torch.empty(B, dtype=torch.int32, device="cuda"),
                     region=torch.empty(B, dtype=torch.int32, device="cuda"), tries=torch.empty(B, dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            getattr(hip_lib, name)(h, B, t["x"].data_ptr(), t["r"].data_ptr(), None if var is None else t["var"].data_ptr(), t["hint"].data_ptr(), 0,
                                   *[o[k].data_ptr() for k in ("u_nom", "x_nom0", "xu_ss", "x_nom", "status", "iters", "region", "tries")])
            hip_lib.synchronize(h)
            assert _bytes({k: v.cpu().numpy() for k, v in o.items()}) == _bytes(host), name
        # clearing: the counters alone, then with the table
        hip_lib.law_hop_stats(h, 0, clear=True)
        assert not hip_lib.law_hop_stats(h, 0).any()
        hip_lib.law_eval(h, X[:8], R[:8], variant=None if var is None else var[:8], hint=hint[:8])
        assert hip_lib.law_hop_stats(h, 0)[TESTS] > 0
        law.clear(0)
        assert not hip_lib.law_hop_stats(h, 0).any()
        # hops off again: today's bytes
        law.set_hops(0)
        if which != "extended":
            hip_lib.law_learn(h, X, R, plain)
            again = hip_lib.law_eval(h, X, R, hint=hint)
            assert _bytes(again) == _bytes(off_h)
    finally:
        mpc._close()


# ------------------------------------------------------------------ 3: the loops
@pytest.fixture(scope="module")
def cart(hip_lib):
    mpc, w = common.make_mpc("cartpole", 10, True, create=True)
    yield mpc, w
    mpc._close()


def _fused_vs_per_step(mpc, law, sc, warm, max_tries, max_hops):
    B, T = sc["th_u"].shape
    outs = []
    for fused in ("on", "off"):
        h0 = law.hits.copy()
        law.hop_stats(clear=True)
        o = _run(mpc, sc, fused=fused, warm_start=warm, capture=B // 2, law=dict(max_tries=max_tries, miss_capacity=B * T, max_hops=max_hops))
        o["region_hits"] = law.hits - h0
        o["hop_stats"] = np.array(list(law.hop_stats().values()), np.int64)
        o["log"] = o["law_misses"]()
        outs.append(o)
    on, off = outs
    assert on["loop_mode"] == 1 and off["loop_mode"] == 0
    _same(on, off, KEYS + LAW_KEYS + ("x_traj", "x_nom_traj", "u_traj", "region_hits", "hop_stats"))
    assert on["log"]["n_total"] == off["log"]["n_total"] and _rows(on["log"]).tobytes() == _rows(off["log"]).tobytes()
    assert int(on["law_hits"].sum()) + on["log"]["n_total"] == B * T and int(on["region_hits"].sum()) == int(on["law_hits"].sum())
    assert on["hop_stats"][TESTS] <= on["law_tries"].sum()
    return on


@pytest.mark.parametrize("warm", [False, True])
def test_fused_equals_per_step_with_hops(hip_lib, cart, warm):
    mpc, w = cart
    law, _ = _learn(mpc, w)
    try:
        for B in (1, 9, 70):
            for T in (1, 2, 12):
                on = _fused_vs_per_step(mpc, law, _scenario(w, B, T), warm, 0, 16)
                st = on["hop_stats"]
                print(f"B {B} T {T} warm {warm}: hit share {on['law_hits'].sum() / (B * T):.3f}, chain hits {st[HITS]}, mean tries {on['law_tries'].sum() / (B * T):.2f}, "
                      f"ended absent {st[ABSENT]} cap {st[CAP]} cycle {st[CYCLE]} parameter row {st[PAR]}")
        _fused_vs_per_step(mpc, law, _scenario(w, 70, 12), warm, 3, 16)
    finally:
        law.set_hops(0)


def test_fused_equals_per_step_with_hops_at_the_long_horizon(hip_lib):
    mpc, w = common.make_mpc("cartpole", 20, True, create=True)
    try:
        law, sc = _learn(mpc, w, B=5, T=4)
        on = _fused_vs_per_step(mpc, law, sc, False, 0, 16)
        assert on["law_hits"].sum() >= 10
    finally:
        mpc._close()


def test_loop_with_hops_log_solved_loop_and_twin(hip_lib, cart):
    """A table with every other region of a pilot over the first half of the sweep: hits, misses and absent neighbours all occur."""
    mpc, w = cart
    B, T = 70, 12
    law, sc = _learn(mpc, w, B, T, pilot_T=6)
    try:
        words = [law.region(i)["words"] for i in range(law.n_regions)]
        law.clear()
        law.add(np.array(words[::2]))
        solved = _run(mpc, sc)
        off = _run(mpc, sc, law=dict(miss_capacity=B * T, max_hops=0))
        law.hop_stats(clear=True)
        out = _run(mpc, sc, law=dict(miss_capacity=B * T, max_hops=16))
        st = np.array(list(law.hop_stats().values()))
        log = out["law_misses"]()
        assert 0 < log["n_total"] < B * T and int(out["law_hits"].sum()) + log["n_total"] == B * T
        assert st[TESTS] > 0 and st[TESTS] <= out["law_tries"].sum()
        # every logged row misses again, hops on and off
        for mh in (16, 0):
            law.set_hops(mh)
            assert np.all(law.evaluate(log["x_k"], log["ref"], max_tries=0, want_traj=False)["region"] == -1)
        _close_to(out, solved)
        assert out["law_hits"].sum() == off["law_hits"].sum()            # (with every candidate allowed a hit is a hit by either search)
        # the host twin: numpy lookups (explicit_law.locate) in the table as the handle holds it, the loop around them on the host, the
        # device's solver behind the misses -- region, tries, hits of EVERY trajectory and the six counters.  (The two loops' states differ
        # by the solver's tolerance carried along; a lookup differs only where a row lies within that of zero, eleven orders below the
        # rows' values.  The bound on the states is asserted first.)
        nc = hip_lib.get_dims(mpc._handle, 0)[1]
        table = [law.region(i) for i in range(law.n_regions)]
        twin = montecarlo.LawPackets.from_tables(mpc.determine_packets, table, mpc.get_steady_state_controller_gain(), 10, ncs=nc, max_hops=16)
        host = montecarlo.run_remote_tube_mpc(twin, w["A"], w["B"], mpc.get_steady_state_controller_gain(), mpc.get_ancillary_controller_gain(), 10,
                                              mpc._Z, sc["p_loss"], sc["ref"], sc["th_u"], sc["ga_u"], sc["w"])
        res = twin.result()
        same = int(np.sum(np.all(out["x_final"] == host["x_final"], axis=1)))
        print(f"hits device {int(out['law_hits'].sum())}, host twin {int(res['law_hits'].sum())} of {B * T}; chain counters device {st.tolist()}, twin "
              f"{res['hop_stats'][0].tolist()}; {same} of {B} final states equal bit for bit")
        _close_to(out, host)
        assert np.array_equal(out["law_hits"], res["law_hits"]) and np.array_equal(out["law_tries"], res["law_tries"])
        assert np.array_equal(out["law_region"], res["law_region"])
        assert np.array_equal(st, res["hop_stats"][0]) and res["misses"]["n_total"] == log["n_total"]
    finally:
        law.set_hops(0)


@pytest.mark.parametrize("form", ["fused", "per_step", "per_step_warm", "stepped", "plants", "series"])
def test_empty_table_with_hops_equals_law_off(hip_lib, cart, form):
    mpc, w = cart
    law = mpc.explicit_law()
    law.clear()
    kw = {"fused": dict(fused="on"), "per_step": dict(fused="off"), "per_step_warm": dict(fused="off", warm_start=True), "stepped": {}, "plants": {},
          "series": dict(series=True, fused="on")}[form]
    try:
        for B, T in ((1, 1), (9, 2), (70, 12)):
            sc = _scenario(w, B, T)
            if form == "plants":
                kw = dict(plant=montecarlo.plant_family("linear", A=np.repeat(w["A"][None], B, 0), B=np.repeat(w["B"][None], B, 0)))
            run = (lambda **k: _stepped(mpc, w, sc, **k)) if form == "stepped" else (lambda **k: _run(mpc, sc, capture=B // 2, **kw, **k))
            off = run()
            on = run(law=dict(miss_capacity=B * T, max_hops=16))
            _same(on, off, KEYS + ("x_traj", "x_nom_traj", "u_traj", "x_violations", "u_violations"))
            assert on["law_misses"]()["n_total"] == B * T and np.all(on["law_tries"] == 0) and not law.hop_stats()["chain_tests"]
    finally:
        law.set_hops(0)


def _wider(mpc, w, B, T, amp, **kw):
    law, sc = _learn(mpc, w, B, T, amp=amp, **kw)
    solved = _run(mpc, sc, **kw)
    off = _run(mpc, sc, law=dict(miss_capacity=B * T, max_hops=0), **kw)
    through = _run(mpc, sc, law=dict(miss_capacity=B * T, max_hops=16), **kw)
    st = sum(np.array(list(law.hop_stats(k).values())) for k in range(mpc._handle.nvariants))
    assert through["loop_mode"] == 0
    n = through["law_misses"]()["n_total"]
    assert int(through["law_hits"].sum()) + n == B * T and through["law_hits"].sum() > 0 and through["law_hits"].sum() == off["law_hits"].sum()
    assert 0 < st[TESTS] <= through["law_tries"].sum()
    _close_to(through, solved)
    law.set_hops(0)
    return through, law


def test_two_input_model_with_hops(hip_lib):
    import test_closed_loop_several_inputs as tsi
    mpc, w = tsi.two_input_mpc(False, device=0)
    try:
        _wider(mpc, w, 9, 6, 2.0, fused="off")
    finally:
        mpc._close()


def test_config5_on_the_block_kernel_with_hops(hip_lib):
    mpc, w = common.make_mpc("synthetic", 30, True, create=True)
    try:
        assert mpc.get_kernel_path() == "block"
        _wider(mpc, w, 4, 3, 1.0)
    finally:
        mpc._close()


def test_extended_controller_with_hops(hip_lib):
    mpc, w = common.make_mpc("cartpole", 10, True, extended=True, create=True)
    try:
        out, law = _wider(mpc, w, 70, 12, 0.5, extended=True, fused="on")
        assert out["law_hits"].sum() >= 0.5 * 70 * 12
    finally:
        mpc._close()


def test_stepped_session_and_plants_with_hops(hip_lib, cart):
    """A session stepped from Python and tmpc_mc_run_plants honour the setting: the chains count, hits + misses are the steps, the loop is
    the solved loop's.  The setter is refused under the open session, which keeps the value it was opened with; set_hops(0) afterwards
    restores today's bytes."""
    mpc, w = cart
    B, T = 9, 12
    law, sc = _learn(mpc, w, B, T)
    L, h = hip_lib.lib(), mpc._handle
    plant = montecarlo.plant_family("linear", A=np.repeat(w["A"][None], B, 0), B=np.repeat(w["B"][None], B, 0))
    try:
        before = _run(mpc, sc, fused="off", law=dict(max_hops=0))
        for form in (lambda **k: _stepped(mpc, w, sc, **k), lambda **k: _run(mpc, sc, plant=plant, **k)):
            solved = form()
            off = form(law=dict(miss_capacity=B * T, max_hops=0))
            law.hop_stats(clear=True)
            on = form(law=dict(miss_capacity=B * T, max_hops=16))
            st = law.hop_stats()
            assert law.max_hops == 0                                      # (the loop's max_hops was the loop's alone)
            assert int(on["law_hits"].sum()) + on["law_misses"]()["n_total"] == B * T and on["law_hits"].sum() == off["law_hits"].sum() > 0
            assert 0 < st["chain_tests"] <= on["law_tries"].sum() and st["chain_hits"] > 0
            _close_to(on, solved)
        x = np.zeros((B, 4))
        with mpc.open_closed_loop(sc["p_loss"], sc["ref"], sc["th_u"], sc["ga_u"], law=dict(max_hops=16)) as s:
            assert L.tmpc_law_set_hops(h.ptr, 0) == -1 and "a stepped closed loop is open on this handle" in h.error()
            assert hip_lib.law_get_hops(h) == 16
            x = x @ w["A"].T + s.step(x) @ w["B"].T + sc["w"][:, 0]
        law.set_hops(0)
        after = _run(mpc, sc, fused="off", law=True)
        _same(after, before, KEYS + LAW_KEYS)
    finally:
        law.set_hops(0)


# ------------------------------------------------------------------ 4: the example
def test_hops_example_runs(hip_lib, capsys, monkeypatch):
    from LinearMPCOverNetworks import polytope_lite as pl
    old = pl.set_lp_backend("hip")           # the examples use the package defaults
    monkeypatch.setattr(sys, "argv", ["explicit_law_hops.py", "--quick"])
    try:
        runpy.run_path(os.path.join(common.ROOT, "examples", "explicit_law_hops.py"), run_name="__main__")
    finally:
        pl.set_lp_backend(old)
    out = capsys.readouterr().out
    assert "hit rate" in out and "the chains" in out and "mean tries" in out and "largest difference of tracking_error" in out
