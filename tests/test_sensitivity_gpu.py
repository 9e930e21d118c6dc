"""The sensitivity kernel (csrc/tmpc_sens.hip) on the GPU: planted QPs through tmpc_qp_sensitivity against the numpy twin and the
long-double judge, the handle entry points against the twin and the un-condensed judge, host and device entries, and the torch layer.

Band of the planted values (the issue's): the kernel's largest error against the judge is at most 10 x the twin's own, with the
floor 1e-12 max|J| under the twin's error -- another elimination order and fused multiply-adds, nothing else, separate the two."""
import os
import runpy
import sys

import numpy as np
import pytest

import common
import sensitivity_reference as sr
from LinearMPCOverNetworks import sensitivity as S
from oracle import qp_sparse
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu
STATES = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
KEYS = ("u_nom", "x_nom0", "xu_ss", "status")
ARGS = ("H", "F", "G", "g0", "Ebar", "Y", "Yp", "P", "Z")


def _both(hip_lib, c, **kw):
    a = [c[k] for k in ARGS]
    return hip_lib.qp_sensitivity(*a, **kw), S.qp_sensitivity(*a, **kw)


def _same_flags(dev, twin, what):
    assert np.array_equal(dev["flag"], twin["flag"]), (what, dev["flag"], twin["flag"])
    assert np.array_equal(dev["n_active"], twin["n_active"]), what
    assert np.array_equal(dev["active"], twin["active"]), what


# ------------------------------------------------------------------ 1: planted cases, both modes
def test_planted_cases_through_the_kernel(hip_lib):
    rng = np.random.default_rng(11)
    worst = (0.0, None)
    for gdef in sr.planted_grid():
        c = sr.planted_case(**gdef)
        J = sr.planted_judge(c)
        floor = 1e-12 * float(np.abs(J).max())
        dev, twin = _both(hip_lib, c)
        _same_flags(dev, twin, gdef)
        assert np.all(dev["flag"] == 0) and np.all(dev["n_active"] == len(c["A"])), gdef
        e_dev = float(np.max(np.abs(dev["out"].astype(np.longdouble) - J[None])))
        e_twin = float(np.max(np.abs(twin["out"].astype(np.longdouble) - J[None])))
        ratio = e_dev / max(e_twin, floor)
        print(f"   {gdef}: kernel {e_dev:.2e}, twin {e_twin:.2e}, ratio {ratio:.2f}")
        worst = max(worst, (ratio, str(gdef)))
        assert e_dev <= 10 * max(e_twin, floor), (gdef, e_dev, e_twin)
        ybar = rng.standard_normal((c["B"], c["ny"]))
        dev, twin = _both(hip_lib, c, mode="vjp", ybar=ybar)
        _same_flags(dev, twin, gdef)
        want = ybar.astype(np.longdouble) @ J
        floor = 1e-12 * float(np.abs(want).max())
        e_dev = float(np.max(np.abs(dev["out"].astype(np.longdouble) - want)))
        e_twin = float(np.max(np.abs(twin["out"].astype(np.longdouble) - want)))
        worst = max(worst, (e_dev / max(e_twin, floor), "vjp " + str(gdef)))
        assert e_dev <= 10 * max(e_twin, floor), ("vjp", gdef, e_dev, e_twin)
    print(f"planted cases: worst kernel error / max(twin error, floor) = {worst[0]:.2f} at {worst[1]}")


@pytest.mark.parametrize("nv", [2, 17, 128])
def test_planted_flags_through_the_kernel(hip_lib, nv):
    nA, nc, npar = nv // 2 + 1, 65 if nv < 128 else 2049, 8
    c = sr.planted_case(50 + nv, nv, nA, nc, npar, 1, weak_row=True)
    dev, twin = _both(hip_lib, c)
    _same_flags(dev, twin, "weak")
    assert dev["flag"][0] == S.WEAK
    c = sr.planted_case(60 + nv, nv, nA, nc, npar, 3, duplicate=True)
    dev, twin = _both(hip_lib, c)
    _same_flags(dev, twin, "duplicate")
    J = sr.planted_judge(c)
    assert np.all(dev["flag"] == S.DEPENDENT) and np.all(dev["active"] == sr.active_words(c["A"], c["nc"])[None])
    e_dev = float(np.max(np.abs(dev["out"].astype(np.longdouble) - J[None])))
    e_twin = float(np.max(np.abs(twin["out"].astype(np.longdouble) - J[None])))
    assert e_dev <= 10 * max(e_twin, 1e-12 * float(np.abs(J).max()))
    c = sr.planted_case(70 + nv, nv, nA, nc, npar, 4)
    c["Z"][1] += 1e-3 * np.random.default_rng(nv).standard_normal(nv)
    c["P"][2, 0] = np.nan
    st = np.array([0, 0, 0, 2], np.int32)
    for mode, ybar in (("jacobian", None), ("vjp", np.ones((4, c["ny"])))):
        dev, twin = _both(hip_lib, c, status=st, mode=mode, ybar=ybar)
        _same_flags(dev, twin, "shifted / NaN / status")
        assert dev["flag"][0] == 0 and dev["flag"][1] & S.NOT_KKT and np.all(np.isfinite(dev["out"][1]))
        assert dev["flag"][2] == S.SKIPPED and dev["flag"][3] == S.SKIPPED and np.all(np.isnan(dev["out"][2:]))
        assert np.allclose(dev["out"][:2], twin["out"][:2], rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------ 2: the handle path against the twin and the judge
def _handle_check(hip_lib, mpc, w, X, R, var, sols, judge_variant=None, n_judge=0):
    h = mpc._handle
    for label, sol in sols:
        sol = {k: sol[k] for k in KEYS}
        dev = hip_lib.sens_jacobian(h, X, R, sol, variant=var)
        twin = S.handle_sensitivity(mpc, X, R, sol, variant=var)
        clean = twin["flag"] == 0
        # the working set is decided by decisive comparisons (slack against act_tol, pivot against rank_tol): equal everywhere, and with it
        # SKIPPED and DEPENDENT.  WEAK and NOT_KKT compare a rounded value with a threshold; where the twin is clean they must agree, and a
        # disagreement elsewhere can only be in those two bits, and in a few instances at most
        assert np.array_equal(dev["n_active"], twin["n_active"]) and np.array_equal(dev["active"], twin["active"]), label
        diff = dev["flag"] ^ twin["flag"]
        assert not np.any(diff & ~np.int32(S.WEAK | S.NOT_KKT)), (label, np.flatnonzero(diff))
        assert not np.any(diff[clean]), (label, np.flatnonzero(diff[clean]))
        assert np.mean(diff == 0) >= 0.97, (label, np.flatnonzero(diff))
        # values: where the working set is well posed -- no flag, or rows dropped by the rank test only -- rounding alone separates kernel and
        # twin (the bound of tests/test_sensitivity.py).  A WEAK / NOT_KKT instance holds a row that is not active at the minimiser, nearly
        # dependent on the others: cond(M) has no bound there and neither has the difference; the values are written and finite
        posed = (twin["flag"] & ~np.int32(S.DEPENDENT)) == 0
        live = (twin["flag"] & S.SKIPPED) == 0
        scale = np.maximum(1.0, np.abs(twin["out"][posed]).max(axis=(1, 2)))
        err = np.abs(dev["J"][posed] - twin["out"][posed]).max(axis=(1, 2)) / scale
        print(f"   {label}: {clean.sum()} of {len(X)} clean, {posed.sum()} well posed, {int((diff != 0).sum())} flag differences, kernel against twin {err.max():.2e}")
        assert err.max() <= 1e-7, label
        assert np.all(np.isfinite(dev["J"][live])), label
        ybar = np.random.default_rng(5).standard_normal((len(X), dev["J"].shape[1]))
        vj = hip_lib.sens_vjp(h, X, R, sol, ybar, variant=var)
        assert np.array_equal(vj["flag"], dev["flag"]) and np.array_equal(vj["n_active"], dev["n_active"]), label
        want = np.einsum("by,byp->bp", ybar[clean], dev["J"][clean])
        assert np.max(np.abs(vj["pbar"][clean] - want) / (1.0 + np.abs(want).max(axis=1, keepdims=True))) <= 1e-9, label
        if n_judge and judge_variant is not None:
            tpl = qp_sparse.SparseTemplate(mpc._problem_dict(), judge_variant)
            done = 0
            for b in np.flatnonzero(clean & ((np.zeros(len(X), int) if var is None else np.asarray(var, dtype=int)) == judge_variant))[:n_judge]:
                j = sr.sparse_jacobian(tpl, (w["A"], w["B"]), X[b], R[b], {k: sol[k][b] for k in KEYS[:3]})
                if j["judged"]:
                    assert np.max(np.abs(dev["J"][b] - j["J"].astype(float))) <= 1e-7 * max(1.0, float(np.abs(j["J"]).max())), (label, b)
                    done += 1
            assert done >= n_judge // 3, (label, done)


@pytest.mark.parametrize("which", ["fixed", "free", "extended"])
def test_cartpole_handles(hip_lib, which):
    X, R = np.ascontiguousarray(STATES[:128, :4]), np.ascontiguousarray(STATES[:128, 4:])
    mpc, w = common.make_mpc("cartpole", 10, which != "free", extended=which == "extended", create=True)
    var = None if which != "extended" else (np.arange(128) % 2).astype(np.uint8)
    own = mpc._solve(X, R, variant=var)
    orc = Oracle(mpc._problem_dict()).solve(X, R, **({} if var is None else dict(variant=var)))
    try:
        _handle_check(hip_lib, mpc, w, X, R, var, (("device's own solutions", own), ("oracle's solutions", orc)),
                      judge_variant=1 if which == "extended" else 0, n_judge=24)
        if which == "extended":
            # an id out of range: SKIPPED, NaN
            bad = var.copy()
            bad[5] = 7
            dev = hip_lib.sens_jacobian(mpc._handle, X, R, {k: own[k] for k in KEYS}, variant=bad)
            assert dev["flag"][5] == S.SKIPPED and np.all(np.isnan(dev["J"][5])) and dev["flag"][4] != S.SKIPPED
    finally:
        mpc._close()


@pytest.mark.parametrize("which", ["two_input", "config5"])
def test_wider_models(hip_lib, which):
    rng = np.random.default_rng(2)
    if which == "two_input":
        import test_closed_loop_several_inputs as tsi
        mpc, w = tsi.two_input_mpc(False, device=0)
    else:
        mpc, w = common.make_mpc("synthetic", 30, True, create=True)
    # interior states and position references, as tests/shape_cases.tracking_states draws them for a model that is not the cart-pole
    nx = mpc._nx
    box = np.asarray(mpc._Xc.b[:nx], dtype=np.float64)
    X = np.ascontiguousarray(rng.uniform(-0.6, 0.6, (32, nx)) * box)
    R = np.ascontiguousarray(np.c_[rng.uniform(-0.8, 0.8, 32) * box[0], np.zeros((32, nx - 1))])
    own = mpc._solve(X, R)
    try:
        assert (own["status"] < 2).sum() >= 16
        _handle_check(hip_lib, mpc, w, X, R, None, (("device's own solutions", own),))
    finally:
        mpc._close()


# ------------------------------------------------------------------ 3: host and device entries
def test_host_and_device_entries_give_equal_bytes(hip_lib):
    """B = 16384: a call lasts far longer than the host needs to enqueue the next one, so that independent calls find unfinished work to
    run beside (the lane counters say where they went), as in tests/test_call_overlap.py."""
    import torch
    B = 16384
    XR = STATES[np.arange(B) % len(STATES)]
    X, R = np.ascontiguousarray(XR[:, :4]), np.ascontiguousarray(XR[:, 4:])
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True)
    try:
        h = mpc._handle
        sol = mpc._solve(X, R, want_traj=False)
        host = hip_lib.sens_jacobian(h, X, R, sol)
        ybar = np.random.default_rng(1).standard_normal((B, host["J"].shape[1]))
        hostv = hip_lib.sens_vjp(h, X, R, sol, ybar)
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(x=X, r=R, u=sol["u_nom"], x0=sol["x_nom0"], ss=sol["xu_ss"], st=sol["status"], yb=ybar).items()}
        nw = hip_lib.sens_active_words(h)
        outs = []
        for rep in range(2):
            o = dict(J=torch.empty(host["J"].shape, dtype=torch.float64, device="cuda"), flag=torch.empty(B, dtype=torch.int32, device="cuda"),
                     na=torch.empty(B, dtype=torch.int32, device="cuda"), act=torch.zeros((B, nw), dtype=torch.int32, device="cuda"),
                     pbar=torch.empty((B, 8), dtype=torch.float64, device="cuda"), flag2=torch.empty(B, dtype=torch.int32, device="cuda"),
                     na2=torch.empty(B, dtype=torch.int32, device="cuda"))
            outs.append(o)
        inputs = (t["x"].data_ptr(), t["r"].data_ptr(), None, t["u"].data_ptr(), t["x0"].data_ptr(), t["ss"].data_ptr(), t["st"].data_ptr(), 0.0)
        torch.cuda.synchronize()
        hip_lib.synchronize(h)
        hip_lib.lane_counters(h, reset=True)
        for o in outs:                    # four successive independent calls (they share what they read only), nothing synchronised in between
            hip_lib.sens_jacobian_device(h, B, *inputs, o["J"].data_ptr(), o["flag"].data_ptr(), o["na"].data_ptr(), o["act"].data_ptr())
            hip_lib.sens_vjp_device(h, B, *inputs, t["yb"].data_ptr(), o["pbar"].data_ptr(), o["flag2"].data_ptr(), o["na2"].data_ptr())
        (n0, n1), waits = hip_lib.lane_counters(h)
        hip_lib.synchronize(h)
        assert n0 + n1 == 4 and n0 >= 1 and n1 >= 1 and waits == 0, (n0, n1, waits)        # both lanes took calls: they ran side by side
        for o in outs:
            assert o["J"].cpu().numpy().tobytes() == host["J"].tobytes()
            assert o["pbar"].cpu().numpy().tobytes() == hostv["pbar"].tobytes()
            assert np.array_equal(o["flag"].cpu().numpy(), host["flag"]) and np.array_equal(o["na"].cpu().numpy(), host["n_active"])
            assert np.array_equal(o["act"].cpu().numpy().view(np.uint32), host["active"])
            assert np.array_equal(o["flag2"].cpu().numpy(), hostv["flag"])
        # a solve of OTHER states that overwrites what an unfinished sensitivity call reads (write after read) stays behind it on its
        # lane: were it to run beside the call, J would be that of a mixture of the two batches
        x2, r2 = torch.roll(t["x"], 7, 0).contiguous(), torch.roll(t["r"], 7, 0).contiguous()
        it = torch.empty(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        hip_lib.lane_counters(h, reset=True)
        hip_lib.sens_jacobian_device(h, B, *inputs, outs[0]["J"].data_ptr(), outs[0]["flag"].data_ptr(), outs[0]["na"].data_ptr(), outs[0]["act"].data_ptr())
        hip_lib.solve_batch_device(h, B, x2.data_ptr(), r2.data_ptr(), None, t["u"].data_ptr(), t["x0"].data_ptr(), t["ss"].data_ptr(), None,
                                   t["st"].data_ptr(), it.data_ptr())
        (m0, m1), _ = hip_lib.lane_counters(h)
        hip_lib.synchronize(h)
        assert (m0, m1) in ((2, 0), (0, 2)), (m0, m1)                  # the dependent solve stayed on the call's lane
        assert outs[0]["J"].cpu().numpy().tobytes() == host["J"].tobytes()
        assert not np.array_equal(t["u"].cpu().numpy(), sol["u_nom"])      # (the solve did write other values)
    finally:
        mpc._close()


def test_refused_while_a_stepped_session_is_open(hip_lib):
    X, R = np.ascontiguousarray(STATES[:4, :4]), np.ascontiguousarray(STATES[:4, 4:])
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True)
    try:
        sol = mpc._solve(X, R)
        rng = np.random.default_rng(0)
        ses = mpc.open_closed_loop(np.full(4, 0.1), np.zeros(5), th_u=rng.uniform(size=(4, 5)), ga_u=rng.uniform(size=(4, 5)))
        try:
            for call in (lambda: hip_lib.sens_jacobian(mpc._handle, X, R, sol), lambda: hip_lib.sens_vjp(mpc._handle, X, R, sol, np.zeros((4, 19)))):
                with pytest.raises(ValueError, match="a stepped closed loop is open on this handle"):
                    call()
        finally:
            ses.close()
        assert np.all(hip_lib.sens_jacobian(mpc._handle, X, R, sol)["flag"] & S.SKIPPED == 0)
    finally:
        mpc._close()


# ------------------------------------------------------------------ 4: the torch layer
def test_mpc_layer_backward(hip_lib):
    import torch
    from LinearMPCOverNetworks.torch_layer import MPCLayer
    X, R = np.ascontiguousarray(STATES[:64, :4]), np.ascontiguousarray(STATES[:64, 4:])
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True)
    try:
        layer = MPCLayer(mpc)
        x = torch.from_numpy(X).cuda().requires_grad_(True)
        r = torch.from_numpy(R).cuda().requires_grad_(True)
        u, x0, ss = layer(x, r)
        gen = torch.Generator(device="cpu").manual_seed(0)
        wu, w0, ws = (torch.randn(t.shape, dtype=torch.float64, generator=gen).cuda() for t in (u, x0, ss))
        ((u * wu).sum() + (x0 * w0).sum() + (ss * ws).sum()).backward()
        assert x.grad is not None and r.grad is not None
        sol = dict(u_nom=u.detach().cpu().numpy(), x_nom0=x0.detach().cpu().numpy(), xu_ss=ss.detach().cpu().numpy(), status=layer.last_status.cpu().numpy())
        jac = hip_lib.sens_jacobian(mpc._handle, X, R, sol)
        ybar = np.c_[wu.cpu().numpy().reshape(64, -1), w0.cpu().numpy(), ws.cpu().numpy()]
        want = np.einsum("by,byp->bp", ybar, jac["J"])
        got = np.c_[x.grad.cpu().numpy(), r.grad.cpu().numpy()]
        assert np.array_equal(layer.last_flag.cpu().numpy(), jac["flag"])
        assert np.max(np.abs(got - want) / (1.0 + np.abs(want).max(axis=1, keepdims=True))) <= 1e-9
        assert np.abs(got[:, :4]).max() > 0 and np.abs(got[:, 4:]).max() > 0         # gradients flow to both inputs
        # finite differences through the layer's own forward where the region is wide (clean flag, step inside the region)
        clean = np.flatnonzero(jac["flag"] == 0)[:24]
        h = 1e-5
        d = np.random.default_rng(4).standard_normal((64, 8))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        ys = []
        with torch.no_grad():
            for s in (1.0, -1.0):
                P = np.c_[X, R] + s * h * d
                uu, xx, sss = layer(torch.from_numpy(np.ascontiguousarray(P[:, :4])).cuda(), torch.from_numpy(np.ascontiguousarray(P[:, 4:])).cuda())
                ys.append(np.c_[uu.cpu().numpy().reshape(64, -1), xx.cpu().numpy(), sss.cpu().numpy()])
                moved = hip_lib.sens_jacobian(mpc._handle, P[:, :4], P[:, 4:], dict(u_nom=uu.cpu().numpy(), x_nom0=xx.cpu().numpy(), xu_ss=sss.cpu().numpy()))
                clean = np.array([b for b in clean if np.array_equal(moved["active"][b], jac["active"][b]) and moved["flag"][b] == 0], dtype=int)
        assert len(clean) >= 8
        fd = (ys[0] - ys[1]) / (2 * h)
        lin = np.einsum("byp,bp->by", jac["J"], d)
        # the solve certifies its answers to 1e-8 of the minimiser: 4 delta / h
        assert np.max(np.abs(fd[clean] - lin[clean])) <= 4 * 1e-8 / h
        # a skipped instance gets a zero gradient and leaves the others alone
        x2 = torch.from_numpy(X).cuda()
        x2[3, 0] = float("nan")
        x2.requires_grad_(True)
        r2 = torch.from_numpy(R).cuda().requires_grad_(True)
        u2, _, _ = layer(x2, r2)
        torch.nan_to_num(u2).sum().backward()
        assert layer.last_flag[3].item() & S.SKIPPED
        assert not x2.grad[3].any() and not r2.grad[3].any() and torch.isfinite(x2.grad).all()
    finally:
        mpc._close()


# ------------------------------------------------------------------ 5: the example
def test_differentiable_mpc_example_runs(hip_lib, capsys, monkeypatch):
    from LinearMPCOverNetworks import polytope_lite as pl
    old = pl.set_lp_backend("hip")           # the examples use the package defaults
    monkeypatch.setattr(sys, "argv", ["differentiable_mpc.py", "--quick"])
    try:
        runpy.run_path(os.path.join(common.ROOT, "examples", "differentiable_mpc.py"), run_name="__main__")
    finally:
        pl.set_lp_backend(old)
    out = capsys.readouterr().out
    assert "distinct critical regions" in out and "cost fell from" in out
