"""A plant model per trajectory (include/tmpc.h: tmpc_mc_set_plant_models for the regulator loop, tmpc_estimate_w_models), the part
that needs no GPU: the exports and their refusals on host-only handles, workloads.cartpole_linearisation, montecarlo.plant_family and
its numpy twins, the host loop on a family of plants with the CPU oracle as the solver, and the W estimate's rollout kernel SOURCE
with a plant per trajectory on the host execution model of tests/wavesim under ASan + UBSan and under MSan
(tests/wavesim/plantsim_main.cpp, through launch_west_rollout itself)."""
import os
import sys

import numpy as np
import pytest

import common
import w_cases
from LinearMPCOverNetworks import _native, montecarlo, workloads
from LinearMPCOverNetworks.control_lite import c2d
from LinearMPCOverNetworks.RegulatorMPC import RegulatorMPC
from oracle.oracle import Oracle
from test_stepped_loop_api import E_DEVICE, E_INVALID

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "wavesim"))
import hostsim  # noqa: E402
import plant_case  # noqa: E402

P = workloads.CARTPOLE_PARAMS
NOMINAL = np.array([P["M"], P["m"], P["b"], P["I"], P["g"], P["l"], 0.02])
LINEAR, CARTPOLE = 0, 1            # include/tmpc.h: TMPC_PLANT_*
PLANT_SEED = 3                     # montecarlo.sample_cartpole: every solve of the host loops below is optimal (found with the CPU oracle)
SPREAD = 0.1


# ------------------------------------------------------------------------------------------------ the C ABI on host-only handles
@pytest.fixture(scope="module")
def handles(hip_lib):
    """Host-only handles (device < 0): the cart-pole tracking controller and a cart-pole regulator."""
    cart, _ = common.make_mpc("cartpole", 10, True, create=True, device=-1)
    w = workloads.cartpole()
    reg = RegulatorMPC(w["A"], w["B"], w["Q"], w["R"], 5)
    reg.set_input_constraints(w["U"])
    reg.set_device(-1)
    reg.generate_optimization_problem()
    yield cart._handle, reg._handle
    cart._close()
    reg._close()


def _set(h, kind, B, models, substeps=10):
    m = None if models is None else np.ascontiguousarray(models, dtype=np.float64)
    rc = _native.lib().tmpc_mc_set_plant_models(h.ptr, kind, B, None if m is None else m.ctypes.data, substeps)
    return rc, h.error()


def _reg_run(reg, B):
    """tmpc_reg_run of B trajectories on a host-only handle: an argument error, or as far as the missing device"""
    x0 = np.zeros((B, 4))
    return _native.lib().tmpc_reg_run(reg.ptr, B, 3, x0.ctypes.data, None, None, None, 0, None, None, 0, None, None, 0, *([None] * 8), -1, None, None, None)


def test_exports_exist_and_are_bound(hip_lib):
    L = _native.lib()
    for name, nargs in (("tmpc_mc_set_plant_models", 5), ("tmpc_estimate_w_models", 30)):
        fn = getattr(L, name)
        assert len(fn.argtypes) == nargs, name
    assert len(L.tmpc_estimate_w.argtypes) == 29 and L.tmpc_abi_version() == _native.ABI_VERSION == 5
    assert L.tmpc_mc_set_plant_models(None, LINEAR, 1, None, 0) == E_INVALID


def test_refusals_name_trajectory_and_entry_and_change_nothing(handles):
    cart, reg = handles
    lin = np.tile(np.c_[workloads.cartpole()["A"], workloads.cartpole()["B"]], (6, 1, 1))
    assert _set(reg, LINEAR, 6, lin)[0] == 0
    assert _reg_run(reg, 2) == E_INVALID and reg.error() == "tmpc_reg_run: B = 2, but the plant models were set for B = 6 trajectories"
    assert _reg_run(reg, 6) == E_DEVICE

    def refused(h, kind, B, models, *words, code=E_INVALID):
        rc, msg = _set(h, kind, B, models)
        assert rc == code and msg.startswith("tmpc_mc_set_plant_models: "), (rc, msg)
        for wd in words:
            assert wd in msg, (wd, msg)

    refused(reg, LINEAR, 3, None, "NULL")
    refused(reg, LINEAR, -1, lin, "B < 0")
    refused(reg, 7, 3, lin, "kind")
    refused(reg, CARTPOLE, 2, np.tile(NOMINAL, (2, 1)), "linear plants only")
    for (i, j), name in (((2, 1), "A[2, 1] of trajectory 1"), ((3, 4), "B[3, 0] of trajectory 1")):
        for bad in (np.nan, np.inf):
            m = lin[:4].copy()
            m[1, i, j] = bad
            refused(reg, LINEAR, 4, m, name, "not finite")
    refused(cart, LINEAR, 6, lin, "only regulator handles", code=-2)          # TMPC_E_UNSUPPORTED: the tracking loops keep their one plant
    # every refusal left the six models in place; B == 0 clears them, and so does plant=None of the Python loop
    assert _reg_run(reg, 2) == E_INVALID and _reg_run(reg, 6) == E_DEVICE
    assert _set(reg, LINEAR, 0, None)[0] == 0 and _reg_run(reg, 2) == E_DEVICE
    assert _native.mc_set_plant_models(reg, "linear", lin) == 6 and _reg_run(reg, 2) == E_INVALID
    assert _native.mc_set_plant_models(reg, "linear", None) is None and _reg_run(reg, 2) == E_DEVICE
    with pytest.raises(ValueError, match="models are"):
        _native.mc_set_plant_models(reg, "linear", lin[:, :, :4])


def test_estimate_w_models_refuses_rows_that_are_no_plant(hip_lib):
    A, B, K = w_cases.scenario()
    for col, name, bad in ((0, "M", 0.0), (0, "M", -1.0), (1, "m", 0.0), (5, "l", 0.0), (5, "l", -0.5), (3, "I", -1e-3), (2, "b", -0.1), (6, "Th", 0.0),
                           (4, "g", np.nan), (0, "M", np.inf), (6, "Th", -np.inf)):
        rows = np.tile(NOMINAL, (4, 1))
        rows[2, col] = bad
        with pytest.raises(RuntimeError, match=r"failed \(-1\): tmpc_estimate_w_models: " + name + " of trajectory 2"):
            _native.estimate_w(A, B, K, 5, x0=np.zeros((4, 4)), par=rows, device=0)
    with pytest.raises(ValueError, match="n_traj, 7"):
        _native.estimate_w(A, B, K, 5, x0=np.zeros((4, 4)), par=np.tile(NOMINAL, (3, 1)), device=0)


# ------------------------------------------------------------------------------------------------ the linearisation
PERTURBED = [dict(M=1.2, m=0.08, b=0.0, I=0.001, g=9.8, l=0.55), dict(M=0.9, m=0.12, b=0.15, I=0.002, g=9.8, l=0.4),
             dict(M=1.05, m=0.1, b=0.05, I=0.0, g=9.81, l=0.62)]


def test_cartpole_linearisation():
    w = workloads.cartpole()
    # the matrices workloads.cartpole() built inline before the linearisation was moved out (results_linear_system.py:26-61), copied
    M, m, b, I, g, l = 1.0, 0.1, 0.0, 0.001, 9.8, 0.5
    p = I * (M + m) + M * m * l ** 2
    Ac0 = np.array([[0, 1, 0, 0], [0, -(I + m * l ** 2) * b / p, -(m ** 2 * g * l ** 2) / p, 0], [0, 0, 0, 1],
                    [0, -(m * l * b) / p, m * g * l * (M + m) / p, 0]], dtype=np.float64)
    Bc0 = np.array([[0], [(I + m * l ** 2) / p], [0], [-m * l / p]], dtype=np.float64)
    A_old, B_old = c2d(Ac0, Bc0, 0.02)
    assert w["A"].tobytes() == A_old.tobytes() and w["B"].tobytes() == B_old.tobytes()
    A, B = workloads.cartpole_linearisation(P, 0.02)
    assert A.tobytes() == w["A"].tobytes() and B.tobytes() == w["B"].tobytes() and A.shape == (4, 4) and B.shape == (4, 1)
    A0, B0 = workloads.cartpole_linearisation()
    assert A0.tobytes() == w["A"].tobytes() and B0.tobytes() == w["B"].tobytes()
    eps, Th = 1e-6, 0.02
    for par in PERTURBED:
        f = lambda x, u: workloads.cartpole_rhs(np.asarray(x, dtype=np.float64), np.array(u), par)      # noqa: E731
        Ac = np.array([(f(np.eye(4)[i] * eps, 0.0) - f(-np.eye(4)[i] * eps, 0.0)) / (2 * eps) for i in range(4)]).T
        Bc = ((f(np.zeros(4), eps) - f(np.zeros(4), -eps)) / (2 * eps)).reshape(4, 1)
        Ad, Bd = c2d(Ac, Bc, Th)
        A, B = workloads.cartpole_linearisation(par, Th)
        np.testing.assert_allclose(A, Ad, atol=1e-9, rtol=0)
        np.testing.assert_allclose(B, Bd, atol=1e-9, rtol=0)
        assert np.max(np.abs(A - w["A"])) > 1e-4                       # it is another plant
    # batched over the leading axes, rows {M, m, b, I, g, l[, Th]} or a dict of arrays
    rows = np.array([[p[k] for k in montecarlo.CARTPOLE_KEYS] + [0.02 + 0.005 * i] for i, p in enumerate(PERTURBED)])
    Ab, Bb = workloads.cartpole_linearisation(rows.reshape(1, 3, 7))
    assert Ab.shape == (1, 3, 4, 4) and Bb.shape == (1, 3, 4, 1)
    for i, p in enumerate(PERTURBED):
        Ai, Bi = workloads.cartpole_linearisation(p, 0.02 + 0.005 * i)
        assert np.array_equal(Ab[0, i], Ai) and np.array_equal(Bb[0, i], Bi)
    Ad, Bd = workloads.cartpole_linearisation({k: rows[:, i] for i, k in enumerate(montecarlo.CARTPOLE_KEYS)}, rows[:, 6])
    assert np.array_equal(Ad, Ab[0]) and np.array_equal(Bd, Bb[0])


# ------------------------------------------------------------------------------------------------ plant_family
def test_plant_family_twins_slices_and_samples():
    rng = np.random.default_rng(8)
    nb = 9
    x, u = rng.uniform(-1, 1, (nb, 4)) * [1.0, 1.0, 0.3, 1.0], rng.uniform(-10, 10, (nb, 1))
    nom = montecarlo.plant_family("cartpole", par=np.tile(NOMINAL, (nb, 1)))
    one = montecarlo.plant_callable("cartpole")
    assert montecarlo.plant_callable(nom) is nom and nom.kind == "cartpole" and len(nom) == nb and nom.models.shape == (nb, 7)
    scale = max(np.abs(one.trace(x, u)).max(), 1.0)
    assert np.max(np.abs(nom(x, u) - one(x, u))) <= 1e-15 * scale and np.max(np.abs(nom.trace(x, u) - one.trace(x, u))) <= 1e-15 * scale
    assert nom.trace(x, u).shape == (11, nb, 4)
    # a dict of scalars and (B,) arrays; missing keys are nominal
    fam = montecarlo.plant_family("cartpole", par=dict(M=np.linspace(0.9, 1.1, nb), l=0.55), Th=0.02, substeps=5)
    assert fam.models.shape == (nb, 7) and np.all(fam.par[:, 5] == 0.55) and np.all(fam.par[:, 1] == P["m"]) and fam.substeps == 5
    assert np.array_equal(fam.par[:, 0], np.linspace(0.9, 1.1, nb))
    for b in (0, 4, 8):                                                # trajectory b is the single plant with its parameters
        par = dict(zip(montecarlo.CARTPOLE_KEYS, fam.par[b, :6]))
        assert np.max(np.abs(fam(x, u)[b] - workloads.cartpole_step(x[b], u[b, 0], 0.02, 5, par))) <= 1e-15 * scale
    # the linear kind
    w = workloads.cartpole()
    lin = montecarlo.plant_family("linear", A=np.tile(w["A"], (nb, 1, 1)), B=np.tile(w["B"], (nb, 1, 1)))
    want = x @ w["A"].T + u @ w["B"].T
    assert np.max(np.abs(lin(x, u) - want)) <= 1e-15 * max(np.abs(want).max(), 1.0) and not hasattr(lin, "trace")
    assert lin.models.shape == (nb, 4, 5) and np.array_equal(lin.models[3], np.c_[w["A"], w["B"]]) and lin.models.flags["C_CONTIGUOUS"]
    A, B = workloads.cartpole_linearisation(fam.par)
    lin = montecarlo.plant_family("linear", A=A, B=B)
    for b in (1, 7):
        assert np.allclose(lin(x, u)[b], A[b] @ x[b] + B[b] @ u[b], rtol=0, atol=1e-15 * 10)
    # slicing commutes with calling
    for f in (fam, lin):
        sl = f[2:7]
        assert len(sl) == 5 and np.array_equal(sl.models, f.models[2:7]) and np.array_equal(sl(x[2:7], u[2:7]), f(x, u)[2:7])
    assert np.array_equal(fam[2:7].trace(x[2:7], u[2:7]), fam.trace(x, u)[:, 2:7]) and fam[2:7].substeps == 5
    # sample_cartpole: keyed by (seed, global trajectory), so a shard is the slice of the whole
    whole = montecarlo.sample_cartpole(40, 0.2, 11)
    part = montecarlo.sample_cartpole(13, 0.2, 11, first=20)
    assert np.array_equal(part.models, whole.models[20:33]) and montecarlo.plant_family.sample_cartpole is montecarlo.sample_cartpole
    par = whole.par
    for col, key in ((0, "M"), (1, "m"), (5, "l")):
        rel = par[:, col] / P[key] - 1.0
        assert np.all(np.abs(rel) <= 0.2 + 1e-15) and np.ptp(rel) > 0.2
    assert np.all(par[:, 2] >= 0.0) and np.all(par[:, 2] < 0.2) and np.ptp(par[:, 2]) > 0.1
    assert np.all(par[:, 3] == P["I"]) and np.all(par[:, 4] == P["g"]) and np.all(par[:, 6] == 0.02)
    assert not np.array_equal(montecarlo.sample_cartpole(40, 0.2, 12).models, whole.models)
    # the Philox words behind it (key (seed, trajectory), counter (0, PLANT_STREAM)): numpy's generator gives the same block
    g = 27
    bitgen = np.random.Philox(key=np.array([11, g], dtype=np.uint64), counter=np.array([2 ** 64 - 1, montecarlo.PLANT_STREAM - 1, 0, 0], dtype=np.uint64))
    words = bitgen.random_raw(4)
    uu = (words >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    assert np.array_equal(par[g, [0, 1, 5]], np.array([P["M"], P["m"], P["l"]]) * (1.0 + 0.2 * (2.0 * uu[:3] - 1.0))) and par[g, 2] == 0.2 * uu[3]


# ------------------------------------------------------------------------------------------------ the host loop
def _oracle_packets(mpc, orc):
    def fn(x_hat, r, gamma=None):
        sol = orc.solve(x_hat, r, gamma)
        u_ss = sol["u_ss"] + sol["x_ss"] @ mpc._K.T                        # TubeTrackingMPC.py:217
        U = np.concatenate([sol["u_nom"], u_ss[:, None, :]], axis=1).transpose(0, 2, 1)
        return np.ascontiguousarray(U), sol["x_nom0"], sol["status"]
    return fn


@pytest.mark.parametrize("extended", [False, True])
def test_host_loop_on_a_family_of_plants(oracle_lib, extended):
    """The cart-pole controller at N = 10 on 24 plants of spread 0.1, both kinds: every solve optimal, and every trajectory ends
    somewhere else than on the nominal plant."""
    nb, T = 24, 40
    mpc, w = common.make_mpc("cartpole", 10, True, extended=extended)
    p_loss = np.tile([0.0, 0.3, 0.6, 0.9], nb // 4)
    th, ga, dist = montecarlo.draw_realisations(nb, T, w["w_bound"], seed=23)
    ref = np.where(np.arange(T) < T // 2, 0.5, -0.3)
    pk = _oracle_packets(mpc, Oracle(mpc._problem_dict()))
    K, Kp = mpc.get_steady_state_controller_gain(), mpc.get_ancillary_controller_gain()
    run = lambda plant: montecarlo.run_remote_tube_mpc(pk, w["A"], w["B"], K, Kp, 10, mpc._Z, p_loss, ref, th, ga, dist,      # noqa: E731
                                                       extended=extended, plant=plant)
    nominal = run(None)
    fam = montecarlo.sample_cartpole(nb, SPREAD, PLANT_SEED)
    A, B = workloads.cartpole_linearisation(fam.par)
    for kind, plant in (("cartpole", fam), ("linear", montecarlo.plant_family("linear", A=A, B=B))):
        out = run(plant)
        assert np.all(out["not_optimal"] == 0), (kind, out["not_optimal"])
        diff = np.abs(out["x_final"] - nominal["x_final"]).max(axis=1)
        print(f"   extended = {extended}, {kind}: min over the trajectories of |x_final - x_final(nominal plant)| = {diff.min():.1e}")
        assert np.all(diff > 1e-5), (kind, diff.min())
        assert ("tracking_error_physics" in out) == (kind == "cartpole")
        assert np.all(np.isfinite(out["tracking_error"])) and out["tracking_error"].max() < 0.2


def test_w_estimate_twin_with_a_plant_per_trajectory():
    A, B, K = w_cases.scenario()
    x0 = montecarlo.draw_initial_states_philox(6, *montecarlo.W_REFERENCE_X0_BOX, seed=456, first=3)
    fam = montecarlo.sample_cartpole(6, 0.2, 5)
    one = montecarlo.estimate_disturbance_box_host(A, B, K, x0, 12)
    same = montecarlo.estimate_disturbance_box_host(A, B, K, x0, 12, par=np.tile(NOMINAL, (6, 1)))
    assert np.max(np.abs(same["samples"] - one["samples"])) <= 1e-15
    out = montecarlo.estimate_disturbance_box_host(A, B, K, x0, 12, par=fam)
    for b in (0, 5):                                                     # trajectory b alone, on its own plant
        alone = montecarlo.estimate_disturbance_box_host(A, B, K, x0[b:b + 1], 12, par=fam[b:b + 1])
        assert np.max(np.abs(alone["samples"][:, :, 0] - out["samples"][:, :, b])) <= 1e-15       # (numpy's sin of one value and of six)
    assert np.abs(out["samples"]).max() > 1.5 * np.abs(one["samples"]).max()       # the mismatch is in the samples: A, B, K stayed nominal
    with pytest.raises(ValueError, match="6 plants"):
        montecarlo.estimate_disturbance_box_host(A, B, K, x0[:4], 12, par=fam)


# ------------------------------------------------------------------------------------------------ the kernels' source on the host model
@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    """The host-model programs under the sanitizers (tests/wavesim/hostsim.py: a host without their runtimes skips, a program that does not
    build fails).  Stand-alone programs: nothing is loaded into Python under a sanitizer."""
    return hostsim.binaries_or_skip(tmp_path_factory, "plantsim")


@pytest.mark.parametrize("build", ["plantsim_asan", "plantsim_msan"])
def test_rollout_with_a_plant_per_trajectory_on_the_host_model(binaries, build):
    """west_rollout_kernel with par_traj: 70 trajectories (a full wave and a second workgroup that is not), every lane on its own seven
    numbers -- the call's own par is poisoned with NaN -- against the numpy twin, in the band of tests/test_w_estimate.py."""
    A, B, K = w_cases.scenario()
    n, T = 70, 6
    fam = montecarlo.sample_cartpole(n, 0.2, 5)
    x0 = montecarlo.draw_initial_states_philox(n, *montecarlo.W_REFERENCE_X0_BOX, seed=456, first=3)
    tw = montecarlo.estimate_disturbance_box_host(A, B, K, x0, T, par=fam)
    for kw in (dict(x0=x0), dict(box=montecarlo.W_REFERENCE_X0_BOX, n_traj=n, seed=456, first=3)):
        out = plant_case.run_rollout(binaries[build], A - B @ K, K, np.full(7, np.nan), fam.models, T, env=hostsim.SAN_ENV, **kw)
        hostsim.assert_clean(out["stderr"])
        assert np.array_equal(out["x0_used"], x0)
        np.testing.assert_allclose(out["samples"], tw["samples"], atol=1e-12, rtol=0)
        np.testing.assert_allclose(out["min"], tw["min"], atol=1e-12, rtol=0)
        np.testing.assert_allclose(out["max"], tw["max"], atol=1e-12, rtol=0)
