"""The explicit-law kernel (csrc/tmpc_law.hip) on the GPU: the clipped family through tmpc_qp_law_eval against the numpy twin and the closed
form, the handle entry points on the cart-pole problems (learn, evaluate, solve with the fallback, reorder), the selector contract of the
fallback, wider models, host and device entries, and the example.

Bounds.  region and tries equal the twin's exactly: the family's margins (tests/law_cases.py) decide every comparison.  y against the
closed form: 1e-11 max|y| (the issue's).  Handle outputs: tests/certificates.certify_outputs unchanged."""
import os
import runpy
import sys

import numpy as np
import pytest

import certificates
import common
import law_cases as lc
from LinearMPCOverNetworks import explicit_law as E

pytestmark = pytest.mark.gpu
STATES = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
OUT = ("u_nom", "x_nom0", "xu_ss", "x_nom", "status", "iters")


# ------------------------------------------------------------------ 1: the clipped family through the handle-free entry
@pytest.mark.parametrize("nc", [1, 63, 64, 65, 2049])
@pytest.mark.parametrize("nv", [1, 17, 128])
def test_clipped_family_through_the_kernel(hip_lib, nv, nc):
    """Every np in {1, 8, 32}, B in {1, 63, 65}, R in {1, 33} and max_tries in {1, 2, 0}; the hints of a batch cycle through a valid id, -1
    and an id out of range.  nc below 2 nv keeps the first nc box rows (one-sided clips), above it padding rows that never bind."""
    calls = hits = 0
    for npar in (1, 8, 32):
        for B in (1, 63, 65):
            c = lc.clipped_case(1000 * nv + 10 * nc + npar + B, nv, nc, npar, B)
            m = c["model"]
            ymax = max(1.0, float(np.abs(c["Z"]).max()))
            for R in (1, 33):
                sets, words = lc.table_of(c, R)
                table = [E.region_law(m, s) for s in sets]
                order = np.random.default_rng(R + B).permutation(R)
                hint = np.array([(b % R, -1, R + 5)[(b + R) % 3] for b in range(B)], np.int32)
                for mt in (1, 2, 0):
                    dev = hip_lib.qp_law_eval(m["H"], m["F"], m["G"], m["g0"], m["Ebar"], m["Y"], m["Yp"], words, order, c["P"], hint=hint, max_tries=mt)
                    region, tries, _ = E.locate(table, c["P"], hint=hint, order=order, max_tries=mt)
                    assert np.array_equal(dev["region"], region) and np.array_equal(dev["tries"], tries), (nv, nc, npar, B, R, mt)
                    hit = region >= 0
                    assert np.all(np.isnan(dev["y"][~hit]))
                    assert np.max(np.abs(dev["y"][hit] - c["Z"][hit]), initial=0.0) <= 1e-11 * ymax, (nv, nc, npar, B, R, mt)
                    calls += 1
                    hits += int(hit.sum())
            # without hints, everything allowed
            dev = hip_lib.qp_law_eval(m["H"], m["F"], m["G"], m["g0"], m["Ebar"], m["Y"], m["Yp"], words, order, c["P"])
            region, tries, _ = E.locate(table, c["P"], order=order)
            assert np.array_equal(dev["region"], region) and np.array_equal(dev["tries"], tries) and region[0] >= 0
    assert calls == 54 and hits > 0
    # a non-finite p and an empty table
    P = c["P"].copy()
    P[0, 0] = np.nan
    dev = hip_lib.qp_law_eval(m["H"], m["F"], m["G"], m["g0"], m["Ebar"], m["Y"], m["Yp"], words, order, P)
    assert dev["region"][0] == -1 and dev["tries"][0] == 0 and np.all(np.isnan(dev["y"][0]))
    dev = hip_lib.qp_law_eval(m["H"], m["F"], m["G"], m["g0"], m["Ebar"], m["Y"], m["Yp"], words[:0], order[:0], c["P"])
    assert np.all(dev["region"] == -1) and np.all(dev["tries"] == 0) and np.all(np.isnan(dev["y"]))


# ------------------------------------------------------------------ 2: cart-pole handles
def _bytes(out):
    return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in OUT)


@pytest.mark.parametrize("which", ["fixed", "free", "extended"])
def test_cartpole_handles(hip_lib, which):
    X, R = np.ascontiguousarray(STATES[:256, :4]), np.ascontiguousarray(STATES[:256, 4:])
    mpc, _ = common.make_mpc("cartpole", 10, which != "free", extended=which == "extended", create=True)
    var = None if which != "extended" else (np.arange(256) % 2).astype(np.uint8)
    try:
        h = mpc._handle
        empty = hip_lib.law_eval(h, X, R, variant=var)                  # an empty table is no error: everything misses
        assert np.all(empty["region"] == -1) and np.all(empty["tries"] == 0) and np.all(empty["status"] == 3) and np.all(np.isnan(empty["u_nom"]))
        plain = mpc._solve(X, R, variant=var)
        ids, n_new = hip_lib.law_learn(h, X, R, plain, variant=var)
        nreg = [len(hip_lib.law_stats(h, k)) for k in range(h.nvariants)]
        assert n_new == sum(nreg) and n_new >= 8 and (ids >= 0).sum() >= 128, (n_new, nreg, (ids >= 0).sum())
        ev = hip_lib.law_eval(h, X, R, variant=var)
        added = ids >= 0
        assert np.all(ev["region"][added] >= 0), np.flatnonzero(ev["region"][added] < 0)      # every instance whose signature was added hits
        hit = ev["region"] >= 0
        assert np.all(ev["status"][hit] == 0) and np.all(ev["iters"][hit] == 0) and np.all(ev["tries"][hit] >= 1)
        assert np.all(ev["status"][~hit] == 3) and np.all(np.isnan(ev["u_nom"][~hit])) and np.all(np.isnan(ev["x_nom"][~hit]))
        hits0 = [hip_lib.law_stats(h, k) for k in range(h.nvariants)]
        assert sum(int(x.sum()) for x in hits0) == int(hit.sum())
        for k in range(h.nvariants):          # the counters are per region
            vk = np.zeros(256, int) if var is None else var
            assert np.array_equal(hits0[k], np.bincount(ev["region"][hit & (vk == k)], minlength=nreg[k]))
        sv = hip_lib.law_solve(h, X, R, variant=var)
        assert np.array_equal(sv["region"], ev["region"]) and np.array_equal(sv["tries"], ev["tries"])
        assert np.all((sv["status"] == 0) | (sv["status"] == 2)) and np.all(sv["iters"][~hit & (sv["status"] == 0)] > 0) and np.all(sv["iters"][hit] == 0)
        cert = certificates.certify_outputs(mpc, X, R, sv, variant=var)
        print(f"{which}: {n_new} regions {nreg}, {int(hit.sum())} of 256 hit, mean tries {ev['tries'].mean():.1f}; certified {cert['n_opt']} optimal, "
              f"{cert['n_inf']} infeasible, worst {cert['worst']}")
        assert cert["n_opt"] >= 128
        # the law's answers and the solver's are the same minimiser
        same = hit & (plain["status"] == 0)
        assert np.max(np.abs(sv["u_nom"][same] - plain["u_nom"][same])) <= 2 * certificates.TOL_U0
        # the right hint: one try
        hinted = hip_lib.law_eval(h, X, R, variant=var, hint=ev["region"])
        assert np.array_equal(hinted["region"], ev["region"]) and np.all(hinted["tries"][hit] == 1)
        assert _bytes(hinted) == _bytes(ev)
        # after reorder: the same bytes, the ids unchanged, no more tries in total
        for k in range(h.nvariants):
            hip_lib.law_reorder(h, k)
        re = hip_lib.law_eval(h, X, R, variant=var)
        assert _bytes(re) == _bytes(ev)
        assert int(re["tries"].sum()) <= int(ev["tries"].sum()), (int(re["tries"].sum()), int(ev["tries"].sum()))
        r0 = hip_lib.law_get_region(h, int(ev["region"][hit][0]), 0 if var is None else int(var[hit][0]))
        p0 = np.r_[X[hit][0], R[hit][0]]
        assert np.all(r0["S"] @ p0 + r0["s"] >= 0.0)
        if which == "extended":               # an id out of range: refused by the kernel, not passed on
            bad = var.copy()
            bad[5] = 7
            o = hip_lib.law_solve(h, X, R, variant=bad)
            assert o["status"][5] == 3 and o["region"][5] == -1 and o["tries"][5] == 0 and np.all(np.isnan(o["u_nom"][5])) and o["status"][4] in (0, 2)
        Xn = X.copy()
        Xn[3, 1] = np.inf
        o = hip_lib.law_solve(h, Xn, R, variant=var)
        assert o["status"][3] == 3 and o["region"][3] == -1 and np.all(np.isnan(o["x_nom"][3])) and o["iters"][3] == 0
    finally:
        mpc._close()


# ------------------------------------------------------------------ 3: the selector contract of the fallback
def test_a_table_half_cleared(hip_lib):
    """Hits carry iters == 0; misses carry the solver's iters > 0 and the solver's bytes: the solve launches behind the law kernel see the
    misses and nothing else."""
    X, R = np.ascontiguousarray(STATES[:256, :4]), np.ascontiguousarray(STATES[:256, 4:])
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True)
    try:
        h = mpc._handle
        plain = mpc._solve(X, R)
        ids, _ = hip_lib.law_learn(h, X, R, plain)
        full = hip_lib.law_eval(h, X, R)
        words = [hip_lib.law_get_region(h, i)["words"] for i in range(int(ids.max()) + 1)]
        hip_lib.law_clear(h)
        assert len(hip_lib.law_stats(h)) == 0
        keep = hip_lib.law_add(h, np.array(words[::2]))                 # every other region, under new ids
        assert np.array_equal(keep, np.arange(len(words[::2])))
        sv = hip_lib.law_solve(h, X, R)
        hit = sv["region"] >= 0
        was = full["region"] >= 0
        even = was & (full["region"] % 2 == 0)              # (their region is still there, behind the same regions as before)
        assert np.all(hit[even]) and not np.any(hit[~was]) and even.sum() >= 16 and (~hit).sum() >= 16
        assert np.array_equal(sv["region"][even], full["region"][even] // 2)
        assert np.all(sv["iters"][hit] == 0) and np.all(sv["iters"][~hit] > 0)
        for k in OUT:
            assert np.ascontiguousarray(sv[k][~hit]).tobytes() == np.ascontiguousarray(plain[k][~hit]).tobytes(), k
            assert np.ascontiguousarray(sv[k][even]).tobytes() == np.ascontiguousarray(full[k][even]).tobytes(), k
        assert hip_lib.last_kernel_ms(h) > 0.0
    finally:
        mpc._close()


# ------------------------------------------------------------------ 4: wider models
@pytest.mark.parametrize("which", ["two_input", "config5"])
def test_wider_models(hip_lib, which):
    rng = np.random.default_rng(2)
    if which == "two_input":
        import test_closed_loop_several_inputs as tsi
        mpc, _ = tsi.two_input_mpc(False, device=0)
    else:
        mpc, _ = common.make_mpc("synthetic", 30, True, create=True)
    nx = mpc._nx
    box = np.asarray(mpc._Xc.b[:nx], dtype=np.float64)
    X = np.ascontiguousarray(rng.uniform(-0.6, 0.6, (32, nx)) * box)
    R = np.ascontiguousarray(np.c_[rng.uniform(-0.8, 0.8, 32) * box[0], np.zeros((32, nx - 1))])
    try:
        h = mpc._handle
        print(f"{which}: kernel {hip_lib.kernel_name(h)}")
        own = mpc._solve(X, R)
        assert (own["status"] < 2).sum() >= 16
        ids, n_new = hip_lib.law_learn(h, X, R, own)
        assert n_new >= 1 and (ids >= 0).sum() >= 16
        ev = hip_lib.law_eval(h, X, R)
        assert np.all(ev["region"][ids >= 0] >= 0)
        sv = hip_lib.law_solve(h, X, R)
        hit = sv["region"] >= 0
        assert np.all(sv["iters"][hit] == 0) and np.all(sv["iters"][~hit & (sv["status"] == 0)] > 0)
        cert = certificates.certify_outputs(mpc, X, R, sv)
        print(f"{which}: {n_new} regions, {int(hit.sum())} of 32 hit; certified {cert['n_opt']} optimal, worst {cert['worst']}")
        assert cert["n_opt"] >= 16
    finally:
        mpc._close()


# ------------------------------------------------------------------ 5: host and device entries
def test_host_and_device_entries_give_equal_bytes(hip_lib):
    """B = 16384, as tests/test_sensitivity_gpu.py: a call lasts longer than the host needs to enqueue the next one, so that independent calls
    find unfinished work to run beside, and the lane counters say where they went."""
    import torch
    B = 16384
    XR = STATES[np.arange(B) % len(STATES)]
    X, R = np.ascontiguousarray(XR[:, :4]), np.ascontiguousarray(XR[:, 4:])
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True)
    try:
        h = mpc._handle
        ids, _ = hip_lib.law_learn(h, X[:300], R[:300], mpc._solve(X[:300], R[:300]))      # part of the states' regions: hits and misses
        host_e, host_s = hip_lib.law_eval(h, X, R), hip_lib.law_solve(h, X, R)
        assert 0 < (host_s["region"] >= 0).sum() < B
        t = dict(x=torch.from_numpy(X).cuda(), r=torch.from_numpy(R).cuda())

        def outs():
            return dict(u_nom=torch.empty((B, 10, 1), dtype=torch.float64, device="cuda"), x_nom0=torch.empty((B, 4), dtype=torch.float64, device="cuda"),
                        xu_ss=torch.empty((B, 5), dtype=torch.float64, device="cuda"), x_nom=torch.empty((B, 11, 4), dtype=torch.float64, device="cuda"),
                        status=torch.empty(B, dtype=torch.int32, device="cuda"), iters=torch.empty(B, dtype=torch.int32, device="cuda"),
                        region=torch.empty(B, dtype=torch.int32, device="cuda"), tries=torch.empty(B, dtype=torch.int32, device="cuda"))

        def ptrs(o):
            return [o[k].data_ptr() for k in ("u_nom", "x_nom0", "xu_ss", "x_nom", "status", "iters", "region", "tries")]

        a, b = outs(), outs()
        torch.cuda.synchronize()
        hip_lib.synchronize(h)
        hip_lib.lane_counters(h, reset=True)
        # two independent calls (they share what they read only), nothing synchronised in between
        hip_lib.law_solve_device(h, B, t["x"].data_ptr(), t["r"].data_ptr(), None, None, 0, *ptrs(a))
        hip_lib.law_eval_device(h, B, t["x"].data_ptr(), t["r"].data_ptr(), None, None, 0, *ptrs(b))
        (n0, n1), waits = hip_lib.lane_counters(h)
        hip_lib.synchronize(h)
        assert n0 == 1 and n1 == 1 and waits == 0, (n0, n1, waits)       # both lanes took a call: they ran side by side
        for k in OUT + ("region", "tries"):
            assert a[k].cpu().numpy().tobytes() == np.ascontiguousarray(host_s[k]).tobytes(), k
            assert b[k].cpu().numpy().tobytes() == np.ascontiguousarray(host_e[k]).tobytes(), k
        # a law call that overwrites the outputs of the unfinished solve before it (write after write) stays behind it on its lane
        x2, r2 = torch.roll(t["x"], 7, 0).contiguous(), torch.roll(t["r"], 7, 0).contiguous()
        torch.cuda.synchronize()
        hip_lib.lane_counters(h, reset=True)
        hip_lib.solve_batch_device(h, B, x2.data_ptr(), r2.data_ptr(), None, a["u_nom"].data_ptr(), a["x_nom0"].data_ptr(), a["xu_ss"].data_ptr(),
                                   a["x_nom"].data_ptr(), a["status"].data_ptr(), a["iters"].data_ptr())
        hip_lib.law_solve_device(h, B, t["x"].data_ptr(), t["r"].data_ptr(), None, None, 0, *ptrs(a))
        (m0, m1), _ = hip_lib.lane_counters(h)
        hip_lib.synchronize(h)
        assert (m0, m1) in ((2, 0), (0, 2)), (m0, m1)
        for k in OUT + ("region", "tries"):
            assert a[k].cpu().numpy().tobytes() == np.ascontiguousarray(host_s[k]).tobytes(), k
    finally:
        mpc._close()


def test_refused_while_a_stepped_session_is_open(hip_lib):
    X, R = np.ascontiguousarray(STATES[:4, :4]), np.ascontiguousarray(STATES[:4, 4:])
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True)
    try:
        h = mpc._handle
        sol = mpc._solve(X, R)
        rng = np.random.default_rng(0)
        ses = mpc.open_closed_loop(np.full(4, 0.1), np.zeros(5), th_u=rng.uniform(size=(4, 5)), ga_u=rng.uniform(size=(4, 5)))
        try:
            for call in (lambda: hip_lib.law_eval(h, X, R), lambda: hip_lib.law_solve(h, X, R), lambda: hip_lib.law_learn(h, X, R, sol),
                         lambda: hip_lib.law_add(h, np.zeros((1, (hip_lib.get_dims(h, 0)[1] + 31) // 32), np.uint32)), lambda: hip_lib.law_reorder(h),
                         lambda: hip_lib.law_clear(h), lambda: hip_lib.law_stats(h)):
                with pytest.raises(ValueError, match="a stepped closed loop is open on this handle"):
                    call()
        finally:
            ses.close()
        law = mpc.explicit_law()
        ids, n_new = law.learn(X, R)
        assert n_new >= 1 and law.n_regions == n_new and np.all(law.solve(X, R)["region"][ids >= 0] >= 0) and int(law.hits.sum()) == int((ids >= 0).sum())
        assert len(law.region(0)["rows"]) == bin(int.from_bytes(law.region(0)["words"].tobytes(), "little")).count("1")
    finally:
        mpc._close()


# ------------------------------------------------------------------ 6: the example
def test_explicit_law_example_runs(hip_lib, capsys, monkeypatch):
    from LinearMPCOverNetworks import polytope_lite as pl
    old = pl.set_lp_backend("hip")           # the examples use the package defaults
    monkeypatch.setattr(sys, "argv", ["explicit_law.py", "--quick"])
    try:
        runpy.run_path(os.path.join(common.ROOT, "examples", "explicit_law.py"), run_name="__main__")
    finally:
        pl.set_lp_backend(old)
    out = capsys.readouterr().out
    assert "hit rate" in out and "regions stored" in out and "largest |u_0 difference|" in out
