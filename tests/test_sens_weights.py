"""Gradients with respect to the weights Q, R, P, T, on the host: the numpy twin (sensitivity.qp_sensitivity_data) against the
long-double judge of tests/sens_weights_reference.py, the weight map (tmpc_sens_weight_map) against the linearity of the condensing,
the twin against central differences of the ORACLE in weight space, the refusals, the kernels' source on the host execution model and
their code-object notes.  The kernels run in tests/test_sens_weights_gpu.py.

Bounds.  * Planted cases: tests/sens_weights_reference.py::bound (its docstring has the reasoning).  pbar and adj against the judge: the
bound of tests/test_sensitivity.py::test_planted_vjp, and the same amplification times the magnitude s_b of the two terms a_b is the
difference of.
* Weight map: the identity  <Wbar, dW> = <Hbar, H(W + dW) - H(W)> + <Fbar, F(W + dW) - F(W)>  is exact in exact arithmetic; every
number in it is a sum of at most n products formed in double, n the longest inner dimension (nv): 8 n EPS times the sum of the
magnitudes of the products on both sides, where the magnitude of a difference H(W + dW) - H(W) is that of its two terms.
* Central differences: (4 delta / h) |ybar|_1 + |fd(h) - fd(2h)| / 3 per instance (the second term estimates the truncation: y is not
affine in W).
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

import common
import sens_weights_reference as wr
import sensitivity_reference as sr
from LinearMPCOverNetworks import sensitivity as S
from oracle import qp_sparse
from oracle.oracle import Oracle

ROOT = os.path.dirname(common.PKG)
STATES = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
EPS = np.finfo(np.float64).eps
KEYS = ("u_nom", "x_nom0", "xu_ss", "status")
ARGS = ("H", "F", "G", "g0", "Ebar", "Y", "Yp", "P", "Z")
WEIGHTS = (("Q", "_Q"), ("R", "_R"), ("P", "_P"), ("T", "_Tout"))
CHUNK = 256           # csrc/tmpc_sens.hpp: SENS_WG_CHUNK


def check_against_judge(c, got, ybar, twin=None, what=""):
    """Hbar, Fbar of `got` within wr.bound of the long-double judge (twice the bound where `twin` is given: got is then another
    implementation of the twin's arithmetic, compared with the twin).  -> the judge."""
    j = wr.judge(c["H"], c["F"], c["G"], c["Ebar"], c["Y"], c["Yp"], c["P"], c["Z"], ybar, c["A"], live=(got["flag"] & S.SKIPPED) == 0)
    bH, bF = wr.bound(wr.amplification(c["H"], c["G"], c["A"]), j["S"], c["P"].shape[0], c["nv"])
    ref, k = (j, 1.0) if twin is None else (twin, 2.0)
    eH = np.abs(got["Hbar"] - ref["Hbar"]).astype(np.float64)
    eF = np.abs(got["Fbar"] - ref["Fbar"]).astype(np.float64)
    print(f"   {what}: Hbar error / bound {np.max(eH / np.maximum(k * bH, 1e-300)):.2e}, Fbar error / bound {np.max(eF / np.maximum(k * bF, 1e-300)):.2e}")
    assert np.all(eH <= k * bH), (what, float(np.max(eH - k * bH)))
    assert np.all(eF <= k * bF), (what, float(np.max(eF - k * bF)))
    return j


# ------------------------------------------------------------------ 1: planted QPs against the long-double judge
def test_planted_cases_against_the_judge():
    rng = np.random.default_rng(21)
    for gdef in sr.planted_grid():
        c = sr.planted_case(**gdef)
        ybar = rng.standard_normal((c["B"], c["ny"]))
        t = S.qp_sensitivity_data(*[c[k] for k in ARGS], ybar)
        assert np.all(t["flag"] == 0) and np.all(t["n_active"] == len(c["A"])), gdef
        assert np.array_equal(t["Hbar"], t["Hbar"].T), gdef
        j = check_against_judge(c, t, ybar, what=str(gdef))
        amp = wr.amplification(c["H"], c["G"], c["A"])
        assert np.all(np.abs(t["adj"] - j["adj"]).max(axis=1) <= amp * j["smag"]), gdef
        J = sr.planted_judge(c)
        assert np.max(np.abs(t["pbar"] - j["pbar"])) <= amp * max(1.0, float(np.abs(J).max())) * c["ny"] * max(1.0, float(np.abs(ybar).max())), gdef
        # the reverse mode is that of qp_sensitivity: the same bytes
        assert t["pbar"].tobytes() == S.qp_sensitivity(*[c[k] for k in ARGS], mode="vjp", ybar=ybar)["out"].tobytes()


def test_skipped_instances_add_nothing():
    c = sr.planted_case(7, 17, 9, 65, 8, 5)
    ybar = np.random.default_rng(0).standard_normal((5, c["ny"]))
    P = c["P"].copy()
    P[2, 1] = np.nan
    st = np.array([0, 0, 2, 0, 0], np.int32)
    a = [c[k] for k in ARGS]
    a[7] = P
    t = S.qp_sensitivity_data(*a, ybar, status=st)
    yb0 = ybar.copy()
    yb0[2] = 0.0
    u = S.qp_sensitivity_data(*[c[k] for k in ARGS], yb0)
    assert t["flag"][2] == S.SKIPPED and not t["adj"][2].any() and np.all(np.isnan(t["pbar"][2]))
    assert np.allclose(t["Hbar"], u["Hbar"], rtol=1e-13, atol=0) and np.allclose(t["Fbar"], u["Fbar"], rtol=1e-13, atol=0)


# ------------------------------------------------------------------ 2: the weight map against the linearity of the condensing
def _bare_tracking():
    from LinearMPCOverNetworks import workloads
    from LinearMPCOverNetworks.TrackingMPC import TrackingMPC
    w = workloads.double_integrator()
    mpc = TrackingMPC(w["A"], w["B"], w["Q"], w["R"], 10)
    mpc.set_input_constraints(w["U"])
    mpc.set_state_constraints(w["X"])
    mpc._Xc, mpc._Uc = mpc._X, mpc._U
    mpc.set_device(-1)
    mpc.generate_optimization_problem(True)
    return mpc


def _host_handle(which):
    if which == "fixed":
        return common.make_mpc("cartpole", 10, True, create=True, device=-1)[0], 0
    if which == "free":
        return common.make_mpc("cartpole", 10, False, create=True, device=-1)[0], 0
    if which == "variant1":
        return common.make_mpc("cartpole", 10, True, extended=True, create=True, device=-1)[0], 1
    if which == "two_input":
        import test_closed_loop_several_inputs as tsi
        return tsi.two_input_mpc(False, device=-1)[0], 0
    return _bare_tracking(), 0


@pytest.mark.parametrize("which", ["fixed", "free", "variant1", "two_input", "terminal_equality"])
def test_weight_map_is_the_adjoint_of_the_condensing(hip_lib, which):
    mpc, k = _host_handle(which)
    try:
        rng = np.random.default_rng(5)
        nv = hip_lib.get_dims(mpc._handle, k)[0]
        Hbar = rng.standard_normal((nv, nv))
        Hbar = Hbar + Hbar.T
        Fbar = rng.standard_normal((nv, 2 * mpc._nx))
        wm = hip_lib.sens_weight_map(mpc._handle, Hbar, Fbar, k)
        if which != "terminal_equality":
            # the long-double map of tests/sens_weights_reference.py, built from the model and the output map alone: sums of nv products
            # with random signs, 8 nv EPS times the magnitude of the same sums (Hbar, Fbar and the signals by their moduli would bound
            # it; the largest entry of the result, eight times over, does for random data)
            m = S.condensed_model(mpc._handle, k)
            ld = wr.weight_map_ld(mpc._A, mpc._B, mpc._handle.N, m["Y"], m["Yp"], Hbar, Fbar)
            for key in ld:
                assert np.max(np.abs(wm[key] - ld[key])) <= 64 * nv * EPS * float(np.abs(ld[key]).max()), (which, key)
        c0 = hip_lib.get_condensed(mpc._handle, k)
        F0 = np.c_[c0["F1"], c0["F2"]]
        for name, attr in WEIGHTS:
            Wbar = wm[name + "bar"]
            assert Wbar.tobytes() == np.ascontiguousarray(Wbar.T).tobytes(), name          # symmetric to the bit
            W = getattr(mpc, attr).copy()
            v = rng.standard_normal(W.shape[0])
            dW = np.outer(v, v)
            dW *= np.linalg.norm(W) / np.linalg.norm(dW)
            mpc.set_cost_weights(**{name: W + dW})
            c1 = hip_lib.get_condensed(mpc._handle, k)
            mpc.set_cost_weights(**{name: W})
            F1 = np.c_[c1["F1"], c1["F2"]]
            lhs = float(np.sum(Wbar * dW))
            rhs = float(np.sum(Hbar * (c1["H"] - c0["H"])) + np.sum(Fbar * (F1 - F0)))
            mag = float(np.sum(np.abs(Wbar) * np.abs(dW)) + np.sum(np.abs(Hbar) * (np.abs(c1["H"]) + np.abs(c0["H"]))) + np.sum(np.abs(Fbar) * (np.abs(F1) + np.abs(F0))))
            print(f"   {which} {name}: <Wbar, dW> = {lhs:.6e}, through the condensing {rhs:.6e}, difference / bound {abs(lhs - rhs) / (8 * nv * EPS * mag):.2e}")
            assert abs(lhs - rhs) <= 8 * nv * EPS * mag, (which, name, lhs, rhs)
            if which == "terminal_equality" and name == "P":
                assert not Wbar.any()
            else:
                assert np.abs(Wbar).max() > 0
        # the weights are back (their symmetric parts: set_cost_weights keeps those)
        assert np.allclose(hip_lib.get_condensed(mpc._handle, k)["H"], c0["H"], rtol=1e-13, atol=0)
    finally:
        mpc._close()


def test_set_cost_weights_keeps_gains_and_sets(hip_lib):
    mpc, _ = common.make_mpc("cartpole", 10, True, extended=True, create=True, device=-1)
    try:
        before = {k: np.array(v) for k, v in mpc._problem_dict().items() if k not in ("Q", "R", "P", "T") and v is not None}
        old = mpc._handle
        mpc.set_cost_weights(Q=2 * mpc._Q, T=3 * mpc._Tout)
        assert mpc._handle is not old and old.ptr is None and mpc._handle.nvariants == 2
        after = mpc._problem_dict()
        assert all(np.array_equal(before[k], after[k]) for k in before)
        with pytest.raises(RuntimeError, match="tmpc_create failed"):
            mpc.set_cost_weights(R=-1e6 * mpc._R)
        assert np.array_equal(mpc._R, after["R"]) and mpc._handle is not None          # the refused weights are not kept
    finally:
        mpc._close()


# ------------------------------------------------------------------ 3: central differences of the oracle in weight space
def wide_states(mpc, w, orc_sol, n=160):
    """The first n golden states whose region is wide: certified, a clean twin flag, every inactive slack and every multiplier above 1e-3.
    -> (indices, the working sets of the un-condensed QP)."""
    X, R = STATES[:, :4], STATES[:, 4:]
    tpl = qp_sparse.SparseTemplate(mpc._problem_dict(), 0)
    twin = S.handle_sensitivity(mpc, X, R, {k: orc_sol[k] for k in KEYS}, mode="vjp", ybar=np.zeros((len(X), 19)))
    wide, sets = [], []
    for b in range(len(X)):
        if len(wide) == n:
            break
        if orc_sol["status"][b] >= 2 or twin["flag"][b] != 0:
            continue
        j = sr.sparse_jacobian(tpl, (w["A"], w["B"]), X[b], R[b], {k: orc_sol[k][b] for k in KEYS[:3]}, want_jacobian=False)
        if j["certified"] and j["min_slack"] > 1e-3 and j["min_mu"] > 1e-3:
            wide.append(b)
            sets.append(j["active"])
    return np.asarray(wide), sets


def oracle_quotients(problem, model, X, R, ybar, sets, name, D, h):
    """Central differences of ybar . y along the weight direction D with steps h and 2h, through the ORACLE.  -> (fd(h), fd(2h), delta,
    same): per instance; same = all four perturbed solves certified on the centre's working set."""
    n = len(X)
    same, delta = np.ones(n, bool), np.zeros(n)
    fd = []
    for step in (h, 2 * h):
        ys = []
        for s in (1.0, -1.0):
            p = dict(problem)
            p[name] = np.ascontiguousarray(problem[name] + s * step * D)
            sol = Oracle(p).solve(X, R)
            tpl = qp_sparse.SparseTemplate(p, 0)
            for i in range(n):
                if sol["status"][i] >= 2:
                    same[i] = False
                    continue
                j = sr.sparse_jacobian(tpl, model, X[i], R[i], {k: sol[k][i] for k in KEYS[:3]}, want_jacobian=False)
                same[i] &= bool(j["certified"]) and np.array_equal(j["active"], sets[i])
                delta[i] = max(delta[i], j["distance"])
            ys.append(np.c_[sol["u_nom"].reshape(n, -1), sol["x_nom0"], sol["xu_ss"]])
        fd.append(np.einsum("by,by->b", ybar, np.nan_to_num(ys[0] - ys[1])) / (2 * step))
    return fd[0], fd[1], delta, same


def check_central_differences(mpc, w, wide, sets, ybar, per_instance, label):
    """per_instance(name) -> (n,) the predicted derivative <Wbar_b, D> of ybar_b . y_b; D from directions()."""
    problem = mpc._problem_dict()
    X, R = np.ascontiguousarray(STATES[wide, :4]), np.ascontiguousarray(STATES[wide, 4:])
    for name, D in directions(mpc).items():
        pred = per_instance(name, D)
        accepted = np.zeros(len(wide), bool)
        todo = np.arange(len(wide))
        worst = 0.0
        for h in (1e-5, 1e-6, 1e-7):
            if not len(todo):
                break
            f1, f2, delta, same = oracle_quotients(problem, (w["A"], w["B"]), X[todo], R[todo], ybar[todo], [sets[i] for i in todo], name, D, h)
            band = 4 * delta / h * np.abs(ybar[todo]).sum(axis=1) + np.abs(f1 - f2) / 3
            err = np.abs(pred[todo] - f1)
            ok = same
            worst = max(worst, float(np.max(err[ok] / band[ok], initial=0.0)))
            assert np.all(err[ok] <= band[ok]), (label, name, h, todo[ok][np.argmax(err[ok] / band[ok])], float(np.max(err[ok] / band[ok])))
            accepted[todo[ok]] = True
            todo = todo[~ok]
        print(f"   {label} {name}: {int(accepted.sum())} of {len(wide)} instances accepted, quotients up to {np.abs(pred).max():.3g}, worst error / band {worst:.3f}")
        assert accepted.sum() >= 150, (label, name, int(accepted.sum()))


def directions(mpc):
    """A random symmetric direction per weight, scaled to the weight's Frobenius norm."""
    rng = np.random.default_rng(17)
    out = {}
    for name, attr in WEIGHTS:
        W = getattr(mpc, attr)
        D = rng.standard_normal(W.shape)
        D = D + D.T
        out[name] = D * (np.linalg.norm(W) / np.linalg.norm(D))
    return out


def test_twin_agrees_with_central_differences_of_the_oracle_in_weight_space(hip_lib, oracle_lib):
    mpc, w = common.make_mpc("cartpole", 10, True, create=True, device=-1)
    try:
        sol = dict(np.load(os.path.join(common.GOLDEN, "cartpole_N10_oracle.npz")))
        wide, sets = wide_states(mpc, w, sol)
        assert len(wide) == 160, len(wide)
        ybar = np.random.default_rng(23).standard_normal((len(wide), 19))
        m = S.condensed_model(mpc)
        X, R = STATES[wide, :4], STATES[wide, 4:]
        Z = S.z_from_outputs(m, X, R, sol["u_nom"][wide], sol["x_nom0"][wide], sol["xu_ss"][wide])
        P = np.c_[X, R]
        t = S.qp_sensitivity_data(m["H"], m["F"], m["G"], m["g0"], m["Ebar"], m["Y"], m["Yp"], P, Z, ybar)
        assert np.all(t["flag"] == 0)
        maps = [hip_lib.sens_weight_map(mpc._handle, -0.5 * (np.outer(a, z) + np.outer(z, a)), -np.outer(a, p)) for a, z, p in zip(t["adj"], Z, P)]
        # the sum of the per-instance gradients is what handle_weight_gradients returns
        total = S.handle_weight_gradients(mpc, X, R, {k: sol[k][wide] for k in KEYS}, ybar)
        for name, _ in WEIGHTS:
            s = sum(mm[name + "bar"] for mm in maps)
            assert np.allclose(total[name + "bar"], s, rtol=1e-9, atol=1e-9 * np.abs(s).max()), name
        check_central_differences(mpc, w, wide, sets, ybar, lambda name, D: np.array([np.sum(mm[name + "bar"] * D) for mm in maps]), "twin")
    finally:
        mpc._close()


# ------------------------------------------------------------------ 4: refusals, on host-only handles
E_INVALID, E_UNSUPPORTED, E_DEVICE = -1, -2, -3
ENTRIES = ("tmpc_sens_vjp_weights", "tmpc_sens_vjp_weights_device")


@pytest.fixture(scope="module")
def handles(hip_lib):
    import regulator_problems
    plain, _ = common.make_mpc("cartpole", 10, True, create=True, device=-1)
    reg = regulator_problems.plain_double_integrator(device=-1)
    lit, _ = common.make_mpc("cartpole", 10, True, extended=True, device=-1)
    lit._eliminate_auxiliaries = False            # the literal terminal row: variant 1 keeps its auxiliaries
    lit.generate_optimization_problem(True)
    yield dict(plain=plain._handle, reg=reg._handle, literal=lit._handle)
    for m in (plain, reg, lit):
        m._close()


def _call(hip_lib, h, name, B=2, null=None, variant=False):
    nx, nu, N = h.nx, h.nu, h.N
    ny = N * nu + 2 * nx + nu
    Bc, B = B, max(B, 1)
    a = dict(x_k=np.zeros((B, nx)), ref=np.zeros((B, nx)), variant=np.zeros(B, np.uint8) if variant else None, u_nom=np.zeros((B, N, nu)),
             x_nom0=np.zeros((B, nx)), xu_ss=np.zeros((B, nx + nu)), status=np.zeros(B, np.int32), ybar=np.zeros((B, ny)),
             pbar=np.zeros((B, 2 * nx)), Q=np.ones((nx, nx)), R=np.ones((nu, nu)), P=np.ones((nx, nx)), T=np.ones((nx, nx)),
             flag=np.zeros(B, np.int32), n_active=np.zeros(B, np.int32))
    if null:
        a[null] = None
    p = {k: (None if v is None else v.ctypes.data) for k, v in a.items()}
    rc = getattr(hip_lib.lib(), name)(h.ptr, Bc, p["x_k"], p["ref"], p["variant"], p["u_nom"], p["x_nom0"], p["xu_ss"], p["status"], 0.0, p["ybar"],
                                      p["pbar"], p["Q"], p["R"], p["P"], p["T"], p["flag"], p["n_active"])
    return rc, h.error(), a


@pytest.mark.parametrize("name", ENTRIES)
def test_null_arguments_are_refused(hip_lib, handles, name):
    for null in ("x_k", "ref", "u_nom", "x_nom0", "xu_ss", "ybar", "pbar", "flag", "n_active"):
        rc, msg, _ = _call(hip_lib, handles["plain"], name, null=null)
        assert rc == E_INVALID and msg == f"{name}: NULL argument", (null, rc, msg)
    assert getattr(hip_lib.lib(), name)(None, 1, *([None] * 7), 0.0, *([None] * 8)) == E_INVALID


@pytest.mark.parametrize("name", ENTRIES)
def test_negative_batch_is_refused_and_an_empty_one_gives_zero_gradients(hip_lib, handles, name):
    rc, msg, _ = _call(hip_lib, handles["plain"], name, B=-1)
    assert rc == E_INVALID and msg == f"{name}: B < 0"
    rc, _, a = _call(hip_lib, handles["plain"], name, B=0)
    assert rc == 0 and not any(a[k].any() for k in "QRPT")


@pytest.mark.parametrize("name", ENTRIES)
def test_host_only_handle_is_refused(hip_lib, handles, name):
    rc, msg, _ = _call(hip_lib, handles["plain"], name)
    assert rc == E_DEVICE and msg == "host-only handle (device < 0): nothing can be solved without the GPU"


@pytest.mark.parametrize("name", ENTRIES)
def test_regulator_handle_is_refused(hip_lib, handles, name):
    rc, msg, _ = _call(hip_lib, handles["reg"], name)
    assert rc == E_UNSUPPORTED and "regulator handle" in msg and msg.startswith(name + ":")


@pytest.mark.parametrize("name", ENTRIES)
def test_auxiliary_variant_is_refused(hip_lib, handles, name):
    rc, msg, _ = _call(hip_lib, handles["literal"], name, variant=True)
    assert rc == E_UNSUPPORTED and "auxiliaries" in msg and msg.startswith(name + ":")
    assert _call(hip_lib, handles["literal"], name)[0] == E_DEVICE          # (variant 0 alone has none)


def test_refusals_of_the_weight_map(hip_lib, handles):
    L = hip_lib.lib()
    h = handles["plain"]
    nv = hip_lib.get_dims(h, 0)[0]
    Hb, Fb, out = np.zeros((nv, nv)), np.zeros((nv, 8)), np.zeros((4, 4))
    assert L.tmpc_sens_weight_map(None, 0, Hb.ctypes.data, Fb.ctypes.data, None, None, None, None) == E_INVALID
    assert L.tmpc_sens_weight_map(h.ptr, 0, None, Fb.ctypes.data, out.ctypes.data, None, None, None) == E_INVALID and h.error() == "tmpc_sens_weight_map: NULL argument"
    assert L.tmpc_sens_weight_map(h.ptr, 1, Hb.ctypes.data, Fb.ctypes.data, None, None, None, None) == E_INVALID and "variant out of range" in h.error()
    assert L.tmpc_sens_weight_map(h.ptr, 0, Hb.ctypes.data, Fb.ctypes.data, None, None, None, None) == 0      # (every output may be NULL)
    r = handles["reg"]
    assert L.tmpc_sens_weight_map(r.ptr, 0, Hb.ctypes.data, Fb.ctypes.data, None, None, None, None) == E_UNSUPPORTED and "regulator handle" in r.error()
    lit = handles["literal"]
    assert L.tmpc_sens_weight_map(lit.ptr, 1, Hb.ctypes.data, Fb.ctypes.data, None, None, None, None) == E_UNSUPPORTED and "auxiliaries" in lit.error()


def test_refusals_of_the_handle_free_entry(hip_lib):
    L = hip_lib.lib()
    c = sr.planted_case(1, 4, 2, 8, 3, 2)
    arr = {k: np.ascontiguousarray(c[k]) for k in ARGS}
    arr.update(ybar=np.zeros((2, 5)), pbar=np.zeros((2, 3)), Hbar=np.ones((4, 4)), Fbar=np.ones((4, 3)), adj=np.zeros((2, 4)), flag=np.zeros(2, np.int32), n_active=np.zeros(2, np.int32))

    def call(device=0, nv=4, nc=8, npar=3, ny=5, B=2, null=None):
        p = {k: v.ctypes.data for k, v in arr.items()}
        if null:
            p[null] = None
        rc = L.tmpc_qp_sensitivity_data(device, nv, nc, npar, ny, p["H"], p["F"], p["G"], p["g0"], p["Ebar"], p["Y"], p["Yp"], B, p["P"], p["Z"], None, 0.0,
                                        p["ybar"], p["pbar"], p["Hbar"], p["Fbar"], p["adj"], p["flag"], p["n_active"])
        return rc, L.tmpc_last_error(None).decode()

    for kw, frag in ((dict(nv=0), "nv = 0 is not in [1, 128]"), (dict(nv=129), "nv = 129"), (dict(npar=33), "np = 33 is not in [1, 32]"), (dict(ny=4097), "ny = 4097"),
                     (dict(nc=-1), "nc = -1"), (dict(B=-1), "B < 0")) + tuple(
                         (dict(null=k), "NULL argument") for k in ("H", "F", "G", "g0", "Ebar", "Y", "Yp", "P", "Z", "ybar", "Hbar", "Fbar", "flag", "n_active")):
        rc, msg = call(**kw)
        assert rc == E_INVALID and msg.startswith("tmpc_qp_sensitivity_data: ") and frag in msg, (kw, rc, msg)
    assert call(B=0)[0] == 0 and not arr["Hbar"].any() and not arr["Fbar"].any()
    rc, msg = call(device=-1)
    assert rc == E_DEVICE and "device < 0" in msg


# ------------------------------------------------------------------ 5: the kernels' source on the host execution model
def run_wgradsim(binary, c, ybar, status=None, env=None):
    """tests/wavesim/wgradsim_main.cpp on a planted case; the instance-independent products as tests/wavesim/sens_case.py forms them."""
    from hostsim import run_files
    H, F, G, g0, Ebar, Y, Yp, P, Z = (np.asarray(c[k], dtype=np.float64) for k in ARGS)
    nv, npar = F.shape
    nc, ny, B = g0.shape[0], Y.shape[0], P.shape[0]
    Hinv = np.linalg.inv(0.5 * (H + H.T))
    Hinv = 0.5 * (Hinv + Hinv.T)
    st = np.zeros(B, np.int32) if status is None else np.asarray(status, dtype=np.int32)
    payload = [np.array([nv, nc, npar, ny, B], dtype=np.int64), np.array([1e-7]), H, Hinv, F, Hinv @ F, G, G @ Hinv, g0, Ebar, Y, Yp, P, Z, st,
               np.asarray(ybar, dtype=np.float64).reshape(B, ny)]
    raw, err = run_files(binary, "run", payload, env)
    sizes = [B * npar, B * nv, nv * nv, nv * npar]
    o = np.frombuffer(raw, dtype=np.float64, count=sum(sizes))
    cut = np.cumsum([0] + sizes)
    flag = np.frombuffer(raw, dtype=np.int32, count=2 * B, offset=8 * sum(sizes))
    assert 8 * sum(sizes) + 8 * B == len(raw)
    return dict(pbar=o[cut[0]:cut[1]].reshape(B, npar).copy(), adj=o[cut[1]:cut[2]].reshape(B, nv).copy(), Hbar=o[cut[2]:cut[3]].reshape(nv, nv).copy(),
                Fbar=o[cut[3]:cut[4]].reshape(nv, npar).copy(), flag=flag[:B].copy(), n_active=flag[B:].copy(), stderr=err)


@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    """The host-model programs under the sanitizers (tests/wavesim/hostsim.py: a host without their runtimes skips, a program that does not
    build fails).  Stand-alone programs: nothing is loaded into Python under a sanitizer."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "wavesim"))
    import hostsim
    return hostsim.binaries_or_skip(tmp_path_factory, "wgradsim")


@pytest.mark.parametrize("build", ["wgradsim_asan", "wgradsim_msan"])
@pytest.mark.parametrize("nv", [1, 17, 128])
def test_kernel_source_on_the_host_model(binaries, build, nv):
    """csrc/tmpc_sens.hip's reverse mode with adj / zrec set, and the reduction, under ASan + UBSan and under MSan: outputs and workspace
    uninitialised, exact-size blocks, B on both sides of the chunk boundaries; one batch with a SKIPPED instance."""
    import hostsim
    for B in (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        # (a working set of half the variables at B = 1; two rows in the long batches, whose subject is the reduction: an instance
        # costs the host model three rendezvous of every thread per working row)
        nA, nc = (1, 3) if nv == 1 else (nv // 2 + 1, 65) if B == 1 else (2, 9)
        c = sr.planted_case(90 + nv, nv, nA, nc, 8 if nv != 17 else 3, B)
        ybar = np.random.default_rng(B).standard_normal((B, c["ny"]))
        status = None
        if B == CHUNK + 1:
            c["P"][CHUNK, 0] = np.nan       # the one instance of the second chunk
            status = np.zeros(B, np.int32)
            status[3] = 2
        out = run_wgradsim(binaries[build], c, ybar, status=status, env=hostsim.SAN_ENV)
        hostsim.assert_clean(out["stderr"])
        twin = S.qp_sensitivity_data(*[c[k] for k in ARGS], ybar, status=status)
        assert np.array_equal(out["flag"], twin["flag"]) and np.array_equal(out["n_active"], twin["n_active"]), (nv, B)
        if status is not None:
            assert out["flag"][3] == S.SKIPPED and out["flag"][CHUNK] == S.SKIPPED and not out["adj"][[3, CHUNK]].any()
        assert out["Hbar"].tobytes() == np.ascontiguousarray(out["Hbar"].T).tobytes()
        check_against_judge(c, out, ybar, what=f"{build} nv {nv} B {B}")


# ------------------------------------------------------------------ 6: the kernels' code objects
def test_code_object_notes(hip_lib):
    spec = importlib.util.spec_from_file_location("code_object_notes", os.path.join(ROOT, "scripts", "code_object_notes.py"))
    notes = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(notes)
    ks = notes.kernels(os.path.join(common.PKG, "lib", "libtmpc_hip.so"))
    dm = notes.demangle(list(ks))
    wg = {dm[n]: k for n, k in ks.items() if "sens_wgrad" in dm[n]}
    assert len(wg) == 2 and any("sens_wgrad_partial_kernel" in n for n in wg) and any("sens_wgrad_sum_kernel" in n for n in wg), sorted(wg)
    for n, k in wg.items():
        assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, (n, k)
        assert k[".vgpr_count"] <= 64 and k[".agpr_count"] == 0 and k[".group_segment_fixed_size"] == 0, (n, k[".vgpr_count"], k[".agpr_count"])
    sens = [k for n, k in ks.items() if "sens_kernel" in dm[n]]
    assert len(sens) == 1
    k = sens[0]            # what tests/test_sensitivity.py asserts, still, with the two pointer tests added
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".vgpr_count"] <= 128 and k[".agpr_count"] == 0
