"""Gradients with respect to the weights on the GPU: the reverse mode of csrc/tmpc_sens.hip with its adj / zrec outputs and the batch
reduction (sens_wgrad_*) through tmpc_qp_sensitivity_data and the handle entries, against the long-double judge of
tests/sens_weights_reference.py, the numpy twin and central differences of the oracle; the torch layer and the example.

Criterion of the values (that of tests/test_sensitivity_gpu.py): the kernel's largest error against the judge is at most 10 x the twin's
own, with the floor 1e-12 max|want| under the twin's error."""
import os
import runpy
import sys

import numpy as np
import pytest

import common
import sens_weights_reference as wr
import sensitivity_reference as sr
import test_sens_weights as tw
from LinearMPCOverNetworks import sensitivity as S

pytestmark = pytest.mark.gpu
STATES = tw.STATES
KEYS, ARGS, CHUNK = tw.KEYS, tw.ARGS, tw.CHUNK
WNAMES = ("Qbar", "Rbar", "Pbar", "Tbar")


def _within(dev, twin, want, what):
    want = np.asarray(want, dtype=np.longdouble)
    e_dev = float(np.max(np.abs(dev.astype(np.longdouble) - want), initial=0.0))
    e_twin = float(np.max(np.abs(twin.astype(np.longdouble) - want), initial=0.0))
    floor = 1e-12 * float(np.max(np.abs(want), initial=0.0))
    print(f"   {what}: kernel {e_dev:.2e}, twin {e_twin:.2e}, floor {floor:.2e}")
    assert e_dev <= 10 * max(e_twin, floor), (what, e_dev, e_twin, floor)


# ------------------------------------------------------------------ 7: planted cases through tmpc_qp_sensitivity_data
def _planted(hip_lib, c, ybar, what):
    a = [c[k] for k in ARGS]
    dev = hip_lib.qp_sensitivity_data(*a, ybar)
    twin = S.qp_sensitivity_data(*a, ybar)
    assert np.array_equal(dev["flag"], twin["flag"]) and np.array_equal(dev["n_active"], twin["n_active"]), what
    assert dev["pbar"].tobytes() == hip_lib.qp_sensitivity(*a, mode="vjp", ybar=ybar)["out"].tobytes(), what
    assert dev["Hbar"].tobytes() == np.ascontiguousarray(dev["Hbar"].T).tobytes(), what
    j = wr.judge(c["H"], c["F"], c["G"], c["Ebar"], c["Y"], c["Yp"], c["P"], c["Z"], ybar, c["A"])
    for key in ("Hbar", "Fbar", "adj"):
        _within(dev[key], twin[key], j[key], f"{what} {key}")
    again = hip_lib.qp_sensitivity_data(*a, ybar)
    assert all(dev[k].tobytes() == again[k].tobytes() for k in ("pbar", "Hbar", "Fbar", "adj", "flag", "n_active")), what
    return dev


@pytest.mark.parametrize("gdef", sr.planted_grid(), ids=lambda g: f"nv{g['nv']}-A{g['nA']}-nc{g['nc']}-np{g['npar']}-B{g['B']}")
def test_planted_grid_through_the_kernels(hip_lib, gdef):
    """With |A| = nv the exact a_b, Hbar and Fbar are zero and so is the floor 1e-12 max|want|: what passes the criterion there is the
    refinement step behind the adj output (a = bv - W_A' M^-1 G_A bv), which leaves kernel and twin at the judge's own rounding."""
    c = sr.planted_case(**gdef)
    _planted(hip_lib, c, np.random.default_rng(gdef["seed"]).standard_normal((c["B"], c["ny"])), str(gdef))


@pytest.mark.parametrize("nv", [1, 17, 128])
def test_batches_around_the_chunk_boundaries(hip_lib, nv):
    nA, nc = (nv // 2 + 1, 65) if nv > 1 else (1, 3)
    for B in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        c = sr.planted_case(90 + nv, nv, nA, nc, 8 if nv != 17 else 3, B)
        _planted(hip_lib, c, np.random.default_rng(B).standard_normal((B, c["ny"])), f"nv {nv} B {B}")


def test_a_skipped_instance_adds_nothing(hip_lib):
    """Status 2 and a NaN in P: the instance is flagged, and Hbar, Fbar are the bytes of the clean batch with that instance's ybar row
    zeroed (its a_b is then an exact zero, and zeros are what the reduction loads for a SKIPPED instance)."""
    B, i = CHUNK + 3, CHUNK + 1
    c = sr.planted_case(97, 17, 9, 65, 8, B)
    ybar = np.random.default_rng(2).standard_normal((B, c["ny"]))
    a = [c[k] for k in ARGS]
    P = c["P"].copy()
    P[i, 2] = np.nan
    st = np.zeros(B, np.int32)
    st[i] = 2
    bad = list(a)
    bad[7] = P
    dev = hip_lib.qp_sensitivity_data(*bad, ybar, status=st)
    yb0 = ybar.copy()
    yb0[i] = 0.0
    clean = hip_lib.qp_sensitivity_data(*a, yb0)
    assert dev["flag"][i] == S.SKIPPED and np.all(np.delete(dev["flag"], i) == 0) and not dev["adj"][i].any() and np.all(np.isnan(dev["pbar"][i]))
    assert not clean["adj"][i].any()
    assert dev["Hbar"].tobytes() == clean["Hbar"].tobytes() and dev["Fbar"].tobytes() == clean["Fbar"].tobytes()
    assert np.all(np.isfinite(dev["Hbar"])) and np.abs(dev["Hbar"]).max() > 0


# ------------------------------------------------------------------ 8, 9: the handle entries
def _judge_on_handle(hip_lib, mpc, X, R, var, sol, ybar):
    """The long-double judge on the handle's condensed data, per variant, on the working sets the twin reports and its own z; every variant's
    (Hbar, Fbar) through the long-double weight map of tests/sens_weights_reference.py, the contributions added."""
    h = mpc._handle
    twin_sets = S.handle_sensitivity(mpc, X, R, sol, variant=var, mode="vjp", ybar=ybar)
    v = np.zeros(len(X), int) if var is None else np.asarray(var, dtype=int)
    want = {k: 0.0 for k in WNAMES}
    for k in range(h.nvariants if var is not None else 1):
        idx = np.flatnonzero(v == k)
        m = S.condensed_model(h, k)
        live = (twin_sets["flag"][idx] & S.SKIPPED) == 0
        # the judge's own z, in long double from what kernel and twin are both given (the solve's outputs): z = Rec [y | p].  (Handed the
        # twin's rounded z instead, the judge would charge the rebuild's rounding to the kernel alone.)
        cat = np.c_[np.nan_to_num(sol["u_nom"][idx]).reshape(len(idx), -1), np.nan_to_num(sol["x_nom0"][idx]), np.nan_to_num(sol["xu_ss"][idx]), X[idx], R[idx]]
        Z = cat.astype(np.longdouble) @ m["Rec"].astype(np.longdouble).T
        sets = list(S.decode_active(twin_sets["active"][idx], nc=m["G"].shape[0]))
        j = wr.judge(m["H"], m["F"], m["G"], m["Ebar"], m["Y"], m["Yp"], np.c_[X[idx], R[idx]], Z, ybar[idx], sets, live=live)
        # mapped to the weights in long double as well: tmpc_sens_weight_map would first round the judge's Hbar, Fbar to double, and a
        # weight gradient is a difference of such terms (Tbar = -2 sum a_theta Mx (x_bar - ref)': small where the reference is reached)
        w = wr.weight_map_ld(mpc._A, mpc._B, h.N, m["Y"], m["Yp"], j["Hbar"], j["Fbar"])
        for key in WNAMES:
            want[key] = want[key] + w[key]
    return want, twin_sets


def _handle_check(hip_lib, mpc, X, R, var, label):
    h = mpc._handle
    sol = {k: v for k, v in mpc._solve(X, R, variant=var, want_traj=False).items() if k in KEYS}
    ny = h.N * h.nu + 2 * h.nx + h.nu
    ybar = np.random.default_rng(5).standard_normal((len(X), ny))
    # a WEAK / NOT_KKT instance holds a row that is nearly dependent on the others: cond(M) has no bound there and neither has the
    # difference between two implementations (tests/test_sensitivity_gpu.py).  Such instances stay in the batch with a zero ybar row.
    flags = S.handle_sensitivity(mpc, X, R, sol, variant=var, mode="vjp", ybar=ybar)["flag"]
    ybar[(flags & ~np.int32(S.DEPENDENT)) != 0] = 0.0
    dev = hip_lib.sens_vjp_weights(h, X, R, sol, ybar, variant=var)
    plain = hip_lib.sens_vjp(h, X, R, sol, ybar, variant=var)
    assert dev["pbar"].tobytes() == plain["pbar"].tobytes() and np.array_equal(dev["flag"], plain["flag"]) and np.array_equal(dev["n_active"], plain["n_active"]), label
    twin = S.handle_weight_gradients(mpc, X, R, sol, ybar, variant=var)
    want, _ = _judge_on_handle(hip_lib, mpc, X, R, var, sol, ybar)
    assert (flags == 0).sum() >= len(X) // 4, (label, int((flags == 0).sum()))
    for key in WNAMES:
        assert dev[key].tobytes() == np.ascontiguousarray(dev[key].T).tobytes(), (label, key)
        _within(dev[key], twin[key], want[key], f"{label} {key}")
    return sol, ybar, dev


@pytest.mark.parametrize("which", ["fixed", "free", "extended"])
def test_cartpole_handles(hip_lib, which):
    import torch
    X, R = np.ascontiguousarray(STATES[:256, :4]), np.ascontiguousarray(STATES[:256, 4:])
    mpc, _ = common.make_mpc("cartpole", 10, which != "free", extended=which == "extended", create=True)
    var = None if which != "extended" else (np.arange(256) % 2).astype(np.uint8)
    try:
        sol, ybar, host = _handle_check(hip_lib, mpc, X, R, var, which)
        if which == "extended":
            assert np.abs(host["Qbar"]).max() > 0
        # the device entry: equal bytes, twice, and the calls counted
        h = mpc._handle
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(x=X, r=R, u=sol["u_nom"], x0=sol["x_nom0"], ss=sol["xu_ss"], st=sol["status"], yb=ybar).items()}
        tv = None if var is None else torch.from_numpy(var).cuda()
        torch.cuda.synchronize()
        hip_lib.synchronize(h)
        hip_lib.lane_counters(h, reset=True)
        for _ in range(2):
            pbar = torch.empty((256, 8), dtype=torch.float64, device="cuda")
            flag = torch.empty(256, dtype=torch.int32, device="cuda")
            na = torch.empty(256, dtype=torch.int32, device="cuda")
            w = hip_lib.sens_vjp_weights_device(h, 256, t["x"].data_ptr(), t["r"].data_ptr(), None if tv is None else tv.data_ptr(), t["u"].data_ptr(), t["x0"].data_ptr(),
                                                t["ss"].data_ptr(), t["st"].data_ptr(), 0.0, t["yb"].data_ptr(), pbar.data_ptr(), flag.data_ptr(), na.data_ptr())
            # (no tmpc_synchronize: the call has synchronised its own lane, pbar and the flags are complete)
            assert all(w[k].tobytes() == host[k].tobytes() for k in WNAMES)
            assert pbar.cpu().numpy().tobytes() == host["pbar"].tobytes() and np.array_equal(flag.cpu().numpy(), host["flag"]) and np.array_equal(na.cpu().numpy(), host["n_active"])
        (n0, n1), waits = hip_lib.lane_counters(h)
        assert n0 + n1 == 2 and waits == 0, (n0, n1, waits)
    finally:
        mpc._close()


def test_wide_states_against_central_differences_of_the_oracle(hip_lib, oracle_lib):
    """The 160 wide golden states of tests/test_sens_weights.py, the device's gradients per instance (a call per instance: the entry sums
    over its batch) within the band of the oracle's central differences in weight space."""
    mpc, w = common.make_mpc("cartpole", 10, True, create=True)
    try:
        sol = dict(np.load(os.path.join(common.GOLDEN, "cartpole_N10_oracle.npz")))
        wide, sets = tw.wide_states(mpc, w, sol)
        assert len(wide) == 160
        ybar = np.random.default_rng(23).standard_normal((len(wide), 19))
        X, R = np.ascontiguousarray(STATES[wide, :4]), np.ascontiguousarray(STATES[wide, 4:])
        per = [hip_lib.sens_vjp_weights(mpc._handle, X[i:i + 1], R[i:i + 1], {k: sol[k][wide[i]:wide[i] + 1] for k in KEYS}, ybar[i:i + 1]) for i in range(len(wide))]
        assert all(p["flag"][0] == 0 for p in per)
        total = hip_lib.sens_vjp_weights(mpc._handle, X, R, {k: sol[k][wide] for k in KEYS}, ybar)
        for key in WNAMES:
            s = sum(p[key] for p in per)
            assert np.allclose(total[key], s, rtol=1e-9, atol=1e-9 * np.abs(s).max()), key
        tw.check_central_differences(mpc, w, wide, sets, ybar, lambda name, D: np.array([np.sum(p[name + "bar"] * D) for p in per]), "device")
    finally:
        mpc._close()


@pytest.mark.parametrize("which", ["two_input", "config5"])
def test_further_shapes(hip_lib, which):
    rng = np.random.default_rng(2)
    if which == "two_input":
        import test_closed_loop_several_inputs as tsi
        mpc, _ = tsi.two_input_mpc(False, device=0)
        B = 32
    else:
        mpc, _ = common.make_mpc("synthetic", 30, True, create=True)
        B = 65
    nx = mpc._nx
    box = np.asarray(mpc._Xc.b[:nx], dtype=np.float64)        # interior states and position references, as tests/test_sensitivity_gpu.py draws them
    X = np.ascontiguousarray(rng.uniform(-0.6, 0.6, (B, nx)) * box)
    R = np.ascontiguousarray(np.c_[rng.uniform(-0.8, 0.8, B) * box[0], np.zeros((B, nx - 1))])
    try:
        if which == "config5":
            assert hip_lib.get_dims(mpc._handle, 0)[0] == 124 and mpc.get_kernel_path() == "block"
        _handle_check(hip_lib, mpc, X, R, None, which)
    finally:
        mpc._close()


# ------------------------------------------------------------------ 10: the torch layer
def test_tunable_layer(hip_lib):
    import torch
    from LinearMPCOverNetworks.torch_layer import TunableMPCLayer
    X, R = np.ascontiguousarray(STATES[:64, :4]), np.ascontiguousarray(STATES[:64, 4:])
    mpc, w = common.make_mpc("cartpole", 10, True, create=True)
    try:
        layer = TunableMPCLayer(mpc)
        assert [tuple(p.shape) for p in layer.parameters()] == [(4, 4), (1, 1), (4, 4), (4, 4)] and all(p.dtype == torch.float64 for p in layer.parameters())
        x = torch.from_numpy(X).cuda().requires_grad_(True)
        r = torch.from_numpy(R).cuda().requires_grad_(True)
        u, x0, ss = layer(x, r)
        gen = torch.Generator(device="cpu").manual_seed(0)
        wu, w0, ws = (torch.randn(t.shape, dtype=torch.float64, generator=gen).cuda() for t in (u, x0, ss))
        ((u * wu).sum() + (x0 * w0).sum() + (ss * ws).sum()).backward()
        sol = dict(u_nom=u.detach().cpu().numpy(), x_nom0=x0.detach().cpu().numpy(), xu_ss=ss.detach().cpu().numpy(), status=layer.last_status.cpu().numpy())
        ybar = np.c_[wu.cpu().numpy().reshape(64, -1), w0.cpu().numpy(), ws.cpu().numpy()]
        want = hip_lib.sens_vjp_weights(mpc._handle, X, R, sol, ybar)
        for p, key in zip((layer.Q, layer.R, layer.P, layer.T), WNAMES):
            assert p.grad is not None and p.grad.numpy().tobytes() == want[key].tobytes(), key
            assert np.abs(want[key]).max() > 0
        skipped = (want["flag"] & S.SKIPPED) != 0
        got = np.c_[x.grad.cpu().numpy(), r.grad.cpu().numpy()]
        assert got[~skipped].tobytes() == want["pbar"][~skipped].tobytes() and not got[skipped].any()
        # an optimiser step: the next forward runs on a new handle, whose outputs are those of a controller built with the new weights
        old = layer.handle
        opt = torch.optim.SGD(layer.parameters(), lr=1e-9)
        opt.step()
        with torch.no_grad():
            u2, x02, ss2 = layer(x, r)
        assert layer.handle is not old and layer.handle is mpc._handle and old.ptr is None
        fresh, _ = common.make_mpc("cartpole", 10, True, create=False)
        fresh.set_cost_weights(*[p.detach().numpy() for p in (layer.Q, layer.R, layer.P, layer.T)])
        fresh.generate_optimization_problem(True)
        try:
            ref = fresh._solve(X, R, want_traj=False)
        finally:
            fresh._close()
        assert np.array_equal(layer.last_status.cpu().numpy(), ref["status"])
        assert u2.cpu().numpy().tobytes() == ref["u_nom"].tobytes() and ss2.cpu().numpy().tobytes() == ref["xu_ss"].tobytes()
        assert not np.array_equal(np.nan_to_num(u2.cpu().numpy()), np.nan_to_num(sol["u_nom"]))          # (the step did move the weights)
        # a weight that makes H indefinite: the library's message
        with torch.no_grad():
            layer.R.copy_(-1e6 * layer.R)
        with pytest.raises(RuntimeError, match="tmpc_create failed"):
            layer(x, r)
    finally:
        mpc._close()


# ------------------------------------------------------------------ 11: the example
def test_learn_weights_example_runs(hip_lib, capsys, monkeypatch):
    from LinearMPCOverNetworks import polytope_lite as pl
    old = pl.set_lp_backend("hip")           # the examples use the package defaults
    monkeypatch.setattr(sys, "argv", ["learn_weights.py", "--quick"])
    try:
        runpy.run_path(os.path.join(common.ROOT, "examples", "learn_weights.py"), run_name="__main__")
    finally:
        pl.set_lp_backend(old)
    out = capsys.readouterr().out
    losses = [float(ln.split("loss")[1].split()[0]) for ln in out.splitlines() if ln.strip().startswith("step")]
    last = float(out.split("steps: loss")[1].split()[0])
    assert len(losses) >= 2 and last < losses[0], out


# ------------------------------------------------------------------ 12: an open session
def test_refused_while_a_stepped_session_is_open(hip_lib):
    X, R = np.ascontiguousarray(STATES[:4, :4]), np.ascontiguousarray(STATES[:4, 4:])
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True)
    try:
        sol = mpc._solve(X, R)
        rng = np.random.default_rng(0)
        ses = mpc.open_closed_loop(np.full(4, 0.1), np.zeros(5), th_u=rng.uniform(size=(4, 5)), ga_u=rng.uniform(size=(4, 5)))
        try:
            with pytest.raises(ValueError, match="a stepped closed loop is open on this handle"):
                hip_lib.sens_vjp_weights(mpc._handle, X, R, sol, np.zeros((4, 19)))
        finally:
            ses.close()
        assert np.all(hip_lib.sens_vjp_weights(mpc._handle, X, R, sol, np.ones((4, 19)))["flag"] & S.SKIPPED == 0)
    finally:
        mpc._close()
