"""Sensitivity of the solution, on the host: the numpy twin of the kernel (LinearMPCOverNetworks/sensitivity.py) against independent
judges (tests/sensitivity_reference.py), the refusals of the C entry points on host-only handles, and the kernel's resource notes.
The kernel itself runs in tests/test_sensitivity_gpu.py.

Bounds.  * Twin against the long-double judge of the un-condensed QP: 1e-7 max(1, |J|_max).  Both differentiate on the same working
set, so only rounding separates them: eps (1.1e-16) times the conditioning of the reduced Hessian (1e5 for the cart-pole, oracle/
qp_sparse.py) times the terminal weight's scale entering F (T = 10 P, |q| ~ 1e6 there) leaves 1e-9 .. 1e-8 relative; two orders above.
* Twin against the planted judge: 8 n eps cond(H) cond(M) max(1, |J|_max), n = nv + |A| -- forming W = G H^-1 costs cond(H), the
products with the explicit M^-1 = L^-T L^-1 cost cond(M), n terms per sum.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

import common
import sensitivity_reference as sr
from LinearMPCOverNetworks import sensitivity as S
from oracle import qp_sparse
from oracle.oracle import Oracle

ROOT = os.path.dirname(common.PKG)
STATES = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
EPS = np.finfo(np.float64).eps
KEYS = ("u_nom", "x_nom0", "xu_ss", "status")


# ------------------------------------------------------------------ 1: the independent judge on the golden states
@pytest.fixture(scope="module")
def golden(hip_lib):
    """Host-only handles of the three cart-pole problems at N = 10, the oracle's solutions of the 600 golden states, the twin's
    Jacobians and the judge's verdicts -- computed once for the tests below."""
    cache = {}

    def get(which):
        if which in cache:
            return cache[which]
        X, R = STATES[:, :4], STATES[:, 4:]
        if which == "fixed":
            mpc, w = common.make_mpc("cartpole", 10, True, create=True, device=-1)
            sol, var, k = dict(np.load(os.path.join(common.GOLDEN, "cartpole_N10_oracle.npz"))), None, 0
        elif which == "free":
            mpc, w = common.make_mpc("cartpole", 10, False, create=True, device=-1)
            sol, var, k = Oracle(mpc._problem_dict()).solve(X, R), None, 0
        else:
            mpc, w = common.make_mpc("cartpole", 10, True, extended=True, create=True, device=-1)
            var, k = np.ones(len(X), np.uint8), 1
            sol = Oracle(mpc._problem_dict()).solve(X, R, variant=var)
        twin = S.handle_sensitivity(mpc, X, R, {kk: sol[kk] for kk in KEYS}, variant=var)
        tpl = qp_sparse.SparseTemplate(mpc._problem_dict(), k)
        judge = [sr.sparse_jacobian(tpl, (w["A"], w["B"]), X[b], R[b], {kk: sol[kk][b] for kk in KEYS[:3]}) if sol["status"][b] < 2
                 else dict(judged=False, J=None, why="not solved", near=False) for b in range(len(X))]
        cache[which] = dict(mpc=mpc, w=w, sol=sol, twin=twin, judge=judge, tpl=tpl)
        return cache[which]

    yield get
    for c in cache.values():
        c["mpc"]._close()


@pytest.mark.parametrize("which", ["fixed", "free", "variant1"])
def test_twin_agrees_with_the_uncondensed_judge(golden, which):
    g = golden(which)
    twin, judge = g["twin"], g["judge"]
    agreed, worst = 0, 0.0
    for b, j in enumerate(judge):
        if j["judged"] and twin["flag"][b] == 0:
            scale = max(1.0, float(np.abs(j["J"]).max()))
            err = float(np.max(np.abs(twin["out"][b].astype(np.longdouble) - j["J"]))) / scale
            worst = max(worst, err)
            assert err <= 1e-7, (which, b, err)
            agreed += 1
        elif not j["judged"]:
            # an instance the judge leaves out carries a flag, or has an inactive row within (1e-7, 1e-5) of its bound
            assert twin["flag"][b] != 0 or j["near"], (which, b, j["why"])
    print(f"{which}: {agreed} of {len(judge)} judged and agreed, worst relative difference {worst:.2e}")
    if which == "fixed":
        assert agreed >= 0.85 * len(judge), agreed
    else:
        assert agreed >= 128, agreed


def test_signature_decodes_to_the_working_set(golden):
    g = golden("fixed")
    m = S.condensed_model(g["mpc"])
    Z = S.z_from_outputs(m, STATES[:, :4], STATES[:, 4:], g["sol"]["u_nom"], g["sol"]["x_nom0"], g["sol"]["xu_ss"])
    rows = S.decode_active(g["twin"]["active"], nc=m["G"].shape[0])
    for b in (0, 17, 333, 599):
        slack = m["g0"] + m["Ebar"] @ STATES[b] - m["G"] @ Z[b]
        assert len(rows[b]) == g["twin"]["n_active"][b]
        assert np.all(slack[rows[b]] <= 1e-7)
        if not g["twin"]["flag"][b] & S.DEPENDENT:
            assert np.array_equal(rows[b], np.flatnonzero(slack <= 1e-7))
    # the output map reproduces the outputs it was inverted from
    y = Z @ m["Y"].T + STATES @ m["Yp"].T
    want = np.c_[g["sol"]["u_nom"].reshape(600, -1), g["sol"]["x_nom0"], g["sol"]["xu_ss"]]
    assert np.max(np.abs(y - want)) < 1e-9


# ------------------------------------------------------------------ 2: central differences of the oracle's solve
def test_twin_agrees_with_central_differences_of_the_oracle(golden):
    """Directional central differences (one direction in x_k, one in ref per instance) of the ORACLE's solve where the region is wide:
    every inactive slack and every multiplier above 1e-3.  Inside a region the law is affine, so the difference quotient is exact up
    to the solver's own error delta: the band is 4 delta / h, delta the largest minimiser_distance among the perturbed solves."""
    g = golden("fixed")
    mpc, w, tpl = g["mpc"], g["w"], g["tpl"]
    orc = Oracle(mpc._problem_dict())
    rng = np.random.default_rng(7)
    wide = []
    for b, j in enumerate(g["judge"]):
        if not (j["judged"] and g["twin"]["flag"][b] == 0):
            continue
        if j["min_slack"] > 1e-3 and j["min_mu"] > 1e-3:
            wide.append(b)
    wide = wide[:160]
    assert len(wide) >= 150, len(wide)
    D = np.zeros((len(wide), 2, 8))
    for i in range(len(wide)):
        D[i, 0, :4] = rng.standard_normal(4)
        D[i, 1, 4:] = rng.standard_normal(4)
        D[i] /= np.linalg.norm(D[i], axis=1, keepdims=True)
    P0 = STATES[wide]
    worst, delta_max, used = 0.0, 0.0, 0
    accepted = np.zeros(len(wide), int)
    steps = {}
    for d in range(2):
        todo = np.arange(len(wide))
        for h in (1e-5, 1e-6, 1e-7):      # a step whose perturbed solves leave the centre's working set is taken again, ten times smaller
            if not len(todo):
                break
            Pp, Pm = P0[todo] + h * D[todo, d], P0[todo] - h * D[todo, d]
            sols = [orc.solve(np.ascontiguousarray(P[:, :4]), np.ascontiguousarray(P[:, 4:])) for P in (Pp, Pm)]
            left = []
            for n, i in enumerate(todo):
                b = wide[i]
                delta, same = 0.0, True
                for P, sol in zip((Pp, Pm), sols):
                    jj = sr.sparse_jacobian(tpl, (w["A"], w["B"]), P[n, :4], P[n, 4:], {kk: sol[kk][n] for kk in KEYS[:3]}, want_jacobian=False)
                    same &= jj["certified"] and np.array_equal(jj["active"], g["judge"][b]["active"])
                    delta = max(delta, jj["distance"])
                if not same:
                    left.append(i)
                    continue
                fd = np.concatenate([(sols[0][kk][n] - sols[1][kk][n]).reshape(-1) for kk in KEYS[:3]]) / (2 * h)
                err = float(np.max(np.abs(g["twin"]["out"][b] @ D[i, d] - fd)))
                band = 4 * delta / h
                worst, delta_max = max(worst, err / band), max(delta_max, delta)
                assert err <= band, (b, d, h, err, band, delta)
                used += 1
                accepted[i] += 1
                steps[h] = steps.get(h, 0) + 1
            todo = np.asarray(left, dtype=int)
    print(f"central differences: {used} directional quotients on {int((accepted > 0).sum())} instances, steps {steps}, largest delta {delta_max:.2e}, "
          f"worst error / band {worst:.3f}")
    assert int((accepted > 0).sum()) >= 150, int((accepted > 0).sum())


# ------------------------------------------------------------------ 3, 4: planted QPs
@pytest.fixture(scope="module")
def planted():
    out = []
    for gdef in sr.planted_grid():
        c = sr.planted_case(**gdef)
        out.append((gdef, c, sr.planted_judge(c)))
    return out


def _planted_bound(c, J):
    A = c["A"]
    M = c["G"][A] @ np.linalg.solve(c["H"], c["G"][A].T) if len(A) else np.eye(1)
    return 8 * (c["nv"] + len(A)) * EPS * np.linalg.cond(c["H"]) * np.linalg.cond(M) * max(1.0, float(np.abs(J).max()))


def test_planted_jacobians(planted):
    for gdef, c, J in planted:
        r = S.qp_sensitivity(c["H"], c["F"], c["G"], c["g0"], c["Ebar"], c["Y"], c["Yp"], c["P"], c["Z"])
        assert np.all(r["flag"] == 0) and np.all(r["n_active"] == len(c["A"])), gdef
        assert np.all(r["active"] == sr.active_words(c["A"], c["nc"])[None]), gdef
        err = float(np.max(np.abs(r["out"].astype(np.longdouble) - J[None])))
        assert err <= _planted_bound(c, J), (gdef, err)
        if len(c["A"]) == 0:
            closed = c["Yp"] - c["Y"] @ np.linalg.solve(c["H"], c["F"])
            assert np.max(np.abs(r["out"] - closed[None])) <= _planted_bound(c, J), gdef


def test_planted_vjp(planted):
    rng = np.random.default_rng(3)
    for gdef, c, J in planted:
        ybar = rng.standard_normal((c["B"], c["ny"]))
        r = S.qp_sensitivity(c["H"], c["F"], c["G"], c["g0"], c["Ebar"], c["Y"], c["Yp"], c["P"], c["Z"], mode="vjp", ybar=ybar)
        want = ybar.astype(np.longdouble) @ J
        err = float(np.max(np.abs(r["out"].astype(np.longdouble) - want)))
        assert np.all(r["flag"] == 0), gdef
        assert err <= _planted_bound(c, J) * c["ny"] * max(1.0, float(np.abs(ybar).max())), (gdef, err)


@pytest.mark.parametrize("nv", [2, 17, 128])
def test_planted_flags(nv):
    nA, nc, npar = nv // 2 + 1, 65 if nv < 128 else 2049, 8
    # a multiplier that is exactly zero: WEAK, the row held active
    c = sr.planted_case(50 + nv, nv, nA, nc, npar, 1, weak_row=True)
    r = S.qp_sensitivity(c["H"], c["F"], c["G"], c["g0"], c["Ebar"], c["Y"], c["Yp"], c["P"], c["Z"])
    assert r["flag"][0] == S.WEAK and r["n_active"][0] == nA
    J = sr.planted_judge(c)
    assert np.max(np.abs(r["out"][0].astype(np.longdouble) - J)) <= _planted_bound(c, J)
    # a duplicated active row: DEPENDENT, and the derivative of the QP without the duplicate
    c = sr.planted_case(60 + nv, nv, nA, nc, npar, 3, duplicate=True)
    r = S.qp_sensitivity(c["H"], c["F"], c["G"], c["g0"], c["Ebar"], c["Y"], c["Yp"], c["P"], c["Z"])
    assert np.all(r["flag"] == S.DEPENDENT) and np.all(r["n_active"] == nA)
    assert np.all(r["active"] == sr.active_words(c["A"], c["nc"])[None])
    J = sr.planted_judge(c)
    assert np.max(np.abs(r["out"].astype(np.longdouble) - J[None])) <= _planted_bound(c, J)
    # a shifted z: NOT_KKT, values still written; a NaN and status = 2: SKIPPED and NaN
    c = sr.planted_case(70 + nv, nv, nA, nc, npar, 4)
    Z, P = c["Z"].copy(), c["P"].copy()
    Z[1] += 1e-3 * np.random.default_rng(nv).standard_normal(nv)
    P[2, 0] = np.nan
    r = S.qp_sensitivity(c["H"], c["F"], c["G"], c["g0"], c["Ebar"], c["Y"], c["Yp"], P, Z, status=np.array([0, 0, 0, 2], np.int32))
    assert r["flag"][0] == 0
    assert r["flag"][1] & S.NOT_KKT and np.all(np.isfinite(r["out"][1]))
    assert r["flag"][2] == S.SKIPPED and r["flag"][3] == S.SKIPPED
    assert np.all(np.isnan(r["out"][2:])) and np.all(r["n_active"][2:] == 0) and not r["active"][2:].any()


# ------------------------------------------------------------------ 5: refusals, on host-only handles
E_INVALID, E_UNSUPPORTED, E_DEVICE = -1, -2, -3


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
             out=np.zeros((B, ny * 2 * nx)), flag=np.zeros(B, np.int32), n_active=np.zeros(B, np.int32), active=np.zeros((B, 64), np.uint32))
    if null:
        a[null] = None
    p = {k: (None if v is None else v.ctypes.data) for k, v in a.items()}
    head = [h.ptr, Bc, p["x_k"], p["ref"], p["variant"], p["u_nom"], p["x_nom0"], p["xu_ss"], p["status"], 0.0]
    tail = [p["ybar"], p["out"], p["flag"], p["n_active"]] if "vjp" in name else [p["out"], p["flag"], p["n_active"], p["active"]]
    rc = getattr(hip_lib.lib(), name)(*head, *tail)
    return rc, h.error()


ENTRIES = ("tmpc_sens_jacobian", "tmpc_sens_jacobian_device", "tmpc_sens_vjp", "tmpc_sens_vjp_device")


@pytest.mark.parametrize("name", ENTRIES)
def test_refusals_of_the_handle_entries(hip_lib, handles, name):
    h = handles["plain"]
    for null in ("x_k", "ref", "u_nom", "x_nom0", "xu_ss", "out", "flag", "n_active") + (("ybar",) if "vjp" in name else ()):
        rc, msg = _call(hip_lib, h, name, null=null)
        assert rc == E_INVALID and msg == f"{name}: NULL argument", (null, rc, msg)
    rc, msg = _call(hip_lib, h, name, B=-1)
    assert rc == E_INVALID and msg == f"{name}: B < 0"
    assert _call(hip_lib, h, name, B=0)[0] == 0
    rc, msg = _call(hip_lib, h, name)
    assert rc == E_DEVICE and msg == "host-only handle (device < 0): nothing can be solved without the GPU"
    rc, msg = _call(hip_lib, handles["reg"], name)
    assert rc == E_UNSUPPORTED and "regulator handle" in msg
    rc, msg = _call(hip_lib, handles["literal"], name, variant=True)
    assert rc == E_UNSUPPORTED and "auxiliaries" in msg
    assert _call(hip_lib, handles["literal"], name)[0] == E_DEVICE          # (variant 0 alone has none)
    assert getattr(hip_lib.lib(), name)(None, 1, *([None] * 7), 0.0, *([None] * 4)) == E_INVALID


def test_refusals_of_the_handle_free_entry(hip_lib):
    L = hip_lib.lib()
    c = sr.planted_case(1, 4, 2, 8, 3, 2)
    arr = {k: np.ascontiguousarray(c[k]) for k in ("H", "F", "G", "g0", "Ebar", "Y", "Yp", "P", "Z")}
    out, flag, nact = np.zeros((2, 5, 3)), np.zeros(2, np.int32), np.zeros(2, np.int32)

    def call(device=0, nv=4, nc=8, npar=3, ny=5, B=2, mode=0, null=None, H=None):
        p = {k: v.ctypes.data for k, v in arr.items()}
        p.update(out=out.ctypes.data, flag=flag.ctypes.data, n_active=nact.ctypes.data)
        if H is not None:
            p["H"] = H.ctypes.data
        if null:
            p[null] = None
        rc = L.tmpc_qp_sensitivity(device, nv, nc, npar, ny, p["H"], p["F"], p["G"], p["g0"], p["Ebar"], p["Y"], p["Yp"], B, p["P"], p["Z"], None, 0.0,
                                   mode, None, p["out"], p["flag"], p["n_active"], None)
        return rc, L.tmpc_last_error(None).decode()

    for kw, frag in ((dict(nv=0), "nv = 0 is not in [1, 128]"), (dict(nv=129), "nv = 129 is not in [1, 128]"), (dict(npar=33), "np = 33 is not in [1, 32]"),
                     (dict(npar=0), "np = 0"), (dict(ny=4097), "ny = 4097"), (dict(ny=0), "ny = 0"), (dict(nc=-1), "nc = -1"), (dict(nc=(1 << 20) + 1), "nc ="),
                     (dict(B=-1), "B < 0"), (dict(mode=2), "mode is"), (dict(mode=1), "NULL argument")) + tuple(
                         (dict(null=k), "NULL argument") for k in ("H", "F", "G", "g0", "Ebar", "Y", "Yp", "P", "Z", "out", "flag", "n_active")):
        rc, msg = call(**kw)
        assert rc == E_INVALID and msg.startswith("tmpc_qp_sensitivity: ") and frag in msg, (kw, rc, msg)
    assert call(B=0)[0] == 0
    rc, msg = call(device=-1)
    assert rc == E_DEVICE and "device < 0" in msg


def test_model_getter_on_a_host_only_handle(hip_lib, handles):
    m = S.condensed_model(handles["plain"])
    c = hip_lib.get_condensed(handles["plain"])
    assert np.array_equal(m["F"], np.c_[c["F1"], c["F2"]]) and np.array_equal(m["Ebar"][:, :4], c["E"]) and not m["Ebar"][:, 4:].any()
    # Rec inverts the output map: Rec [Y z + Yp p | p] = z
    rng = np.random.default_rng(0)
    z, p = rng.standard_normal(m["Y"].shape[1]), rng.standard_normal(8)
    assert np.max(np.abs(m["Rec"] @ np.r_[m["Y"] @ z + m["Yp"] @ p, p] - z)) < 1e-10
    assert hip_lib.lib().tmpc_sens_get_model(handles["reg"].ptr, 0, None, None, None, None, None) == E_UNSUPPORTED


# ------------------------------------------------------------------ 6: the kernel's source on the host execution model
@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    """The host-model programs under the sanitizers (tests/wavesim/hostsim.py: a host without their runtimes skips, a program that does not
    build fails).  Stand-alone programs: nothing is loaded into Python under a sanitizer."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "wavesim"))
    import hostsim
    import sens_case
    return sens_case, hostsim.binaries_or_skip(tmp_path_factory, "senssim")


@pytest.mark.parametrize("build", ["senssim_asan", "senssim_msan"])
@pytest.mark.parametrize("nv", [1, 17, 128])
def test_kernel_source_on_the_host_model(binaries, build, nv):
    """csrc/tmpc_sens.hip compiled for the CPU under ASan + UBSan and under MSan, outputs and workspace uninitialised, exact-size blocks:
    planted cases in both modes (64 and 256 threads, rows across the chunk boundary at nv = 128), the flags, against the twin."""
    import hostsim
    sens_case, bins = binaries
    nA, nc = (nv // 2 + 1, 65 if nv < 128 else 600) if nv > 1 else (1, 3)
    cases = [(sr.planted_case(80 + nv, nv, nA, nc, 8, 3), None)]
    if nv > 1:
        cases.append((sr.planted_case(81 + nv, nv, nA, nc, 3, 2, duplicate=True), None))
        cases.append((sr.planted_case(82 + nv, nv, nv, nc, 1, 1, weak_row=True), None))
        c = sr.planted_case(83 + nv, nv, nA, nc, 8, 4)
        c["Z"][1] += 1e-3 * np.random.default_rng(nv).standard_normal(nv)
        c["P"][2, 0] = np.nan
        cases.append((c, np.array([0, 0, 0, 2], np.int32)))
    for c, status in cases:
        a = [c[k] for k in ("H", "F", "G", "g0", "Ebar", "Y", "Yp", "P", "Z")]
        ybar = np.random.default_rng(1).standard_normal((c["P"].shape[0], c["ny"]))
        for mode in ("jacobian", "vjp"):
            out = sens_case.run(bins[build], *a, status=status, mode=mode, ybar=ybar, env=hostsim.SAN_ENV)
            hostsim.assert_clean(out["stderr"])
            twin = S.qp_sensitivity(*a, status=status, mode=mode, ybar=ybar)
            assert np.array_equal(out["flag"], twin["flag"]) and np.array_equal(out["n_active"], twin["n_active"]) and np.array_equal(out["active"], twin["active"])
            ok = twin["flag"] != S.SKIPPED
            assert np.all(np.isnan(out["out"][~ok]))
            J = sr.planted_judge(c)
            scale = _planted_bound(c, J) * (c["ny"] * max(1.0, float(np.abs(ybar).max())) if mode == "vjp" else 1.0)
            assert np.max(np.abs(out["out"][ok] - twin["out"][ok]), initial=0.0) <= 2 * scale, (nv, mode)


# ------------------------------------------------------------------ the kernel's code object
def test_sensitivity_kernel_has_no_scratch(hip_lib):
    spec = importlib.util.spec_from_file_location("code_object_notes", os.path.join(ROOT, "scripts", "code_object_notes.py"))
    notes = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(notes)
    ks = notes.kernels(os.path.join(common.PKG, "lib", "libtmpc_hip.so"))
    dm = notes.demangle(list(ks))
    sens = {dm[n]: k for n, k in ks.items() if "sens_kernel" in dm[n]}
    assert len(sens) == 1, sorted(sens)
    for n, k in sens.items():
        assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0, (n, k[".private_segment_fixed_size"], k[".vgpr_spill_count"])
        assert k[".vgpr_count"] <= 128 and k[".agpr_count"] == 0, (n, k[".vgpr_count"], k[".agpr_count"])     # four waves per SIMD
        # none of the name filters of tests/test_code_objects.py catches it
        assert not any(f in n for f in ("::solve_kernel<", "::closed_loop", "::solve_block_kernel<", "mc_step_kernel", "::lp_kernel<")), n
