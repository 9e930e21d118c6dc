"""A plant per trajectory in the tracking loops (include/tmpc.h: tmpc_mc_run_plants, tmpc_plant_step_device), the part that needs no GPU:
the exports, every refusal of the two entry points on host-only handles, and the plant kernels' SOURCE (csrc/tmpc_plant.hip) on the host
execution model of tests/wavesim under ASan + UBSan and under MSan (tests/wavesim/plantstep_main.cpp, through launch_plant_step itself)
against the numpy twin montecarlo.PlantFamily.__call__."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import common
from LinearMPCOverNetworks import _native, montecarlo, workloads
from LinearMPCOverNetworks.RegulatorMPC import RegulatorMPC
from test_plant_models import NOMINAL
from test_stepped_loop_api import E_DEVICE, E_INVALID

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "wavesim"))
import hostsim  # noqa: E402
import plantstep_case  # noqa: E402

LINEAR, CARTPOLE = 0, 1            # include/tmpc.h: TMPC_PLANT_*
EPS = np.finfo(np.float64).eps
# The cart-pole kernel against the numpy twin: the tolerance tests/test_plant_models.py:293-295 applies to the W estimate's rollout on the
# same model (mcstep::cartpole_rhs, the same RK4) against the same twin (workloads.cartpole_trace).  It is a literal there, so it cannot be
# imported; it is repeated, not chosen.
CARTPOLE_ATOL = 1e-12


def linear_bound(fam, x, u, w=None):
    """|dev - numpy| <= 2 (nx + nu + 1) eps (sum_k |A_ik| |x_k| + sum_j |B_ij| |u_j| + |w_i|) per component: both sides sum the same
    nx + nu + 1 terms, each side with a relative error below (nx + nu + 1) eps of the sum of magnitudes (fused or not, any order)."""
    nx, nu = fam.A.shape[1], fam.B.shape[2]
    mag = np.einsum("bij,bj->bi", np.abs(fam.A), np.abs(x)) + np.einsum("bij,bj->bi", np.abs(fam.B), np.abs(u))
    if w is not None:
        mag = mag + np.abs(w)
    return 2.0 * (nx + nu + 1) * EPS * mag


def linear_family(nb, nx, nu, seed):
    rng = np.random.default_rng(seed)
    return montecarlo.plant_family("linear", A=rng.uniform(-1, 1, (nb, nx, nx)), B=rng.uniform(-1, 1, (nb, nx, nu)))


# ------------------------------------------------------------------------------------------------ the C ABI on host-only handles
@pytest.fixture(scope="module")
def handles(hip_lib):
    """Host-only handles (device < 0): the cart-pole tracking controller, the double integrator's (nx = 2, nu = 1) and a cart-pole regulator."""
    cart, _ = common.make_mpc("cartpole", 10, True, create=True, device=-1)
    di, _ = common.make_mpc("double_integrator", 5, True, create=True, device=-1)
    w = workloads.cartpole()
    reg = RegulatorMPC(w["A"], w["B"], w["Q"], w["R"], 5)
    reg.set_input_constraints(w["U"])
    reg.set_device(-1)
    reg.generate_optimization_problem()
    yield cart._handle, di._handle, reg._handle
    for m in (cart, di, reg):
        m._close()


def raw_run(h, B, T, kind, models, substeps=10, extended=0, p_loss=True, ref=True, th=True, ga=True, w=True):
    """tmpc_mc_run_plants with plain arrays -> (return code, message).  True: zeros of the right size; None: NULL."""
    keep = []

    def arr(v, shape):
        if v is None:
            return None
        a = np.zeros(shape) if v is True else np.ascontiguousarray(v, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data
    nb, nt = max(B, 1), max(T, 1)
    rc = _native.lib().tmpc_mc_run_plants(h.ptr, B, T, extended, kind, arr(models, None), substeps, arr(p_loss, nb), arr(ref, nt), arr(th, (nb, nt)),
                                          arr(ga, (nb, nt)), arr(w, (nb, nt, h.nx)), None, None, None, 0, None, None, 0, None, None, 0, *([None] * 9))
    return rc, h.error()


def test_exports_exist_and_are_bound(hip_lib):
    L = _native.lib()
    for name, nargs in (("tmpc_mc_run_plants", 31), ("tmpc_plant_step_device", 12)):
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, name
    assert callable(_native.mc_run_plants) and callable(_native.plant_step) and L.tmpc_abi_version() == _native.ABI_VERSION == 5
    assert L.tmpc_mc_run_plants(None, 1, 1, 0, CARTPOLE, None, 10, *([None] * 6), *([None, None, 0] * 3), *([None] * 9)) == E_INVALID
    src = open(common.ROOT + "/include/tmpc.h").read()
    assert "int tmpc_mc_run_plants(" in src and "int tmpc_plant_step_device(" in src


def test_run_plants_refusals_on_host_only_handles(handles):
    cart, di, reg = handles
    rows = np.tile(NOMINAL, (6, 1))
    w2 = common.workload("double_integrator")
    lin2 = np.tile(np.c_[w2["A"], w2["B"]], (6, 1, 1))

    def refused(h, B, T, kind, models, *words, **kw):
        rc, msg = raw_run(h, B, T, kind, models, **kw)
        assert rc == E_INVALID and msg.startswith("tmpc_mc_run_plants: "), (rc, msg)
        for wd in words:
            assert wd in msg, (wd, msg)

    # a valid call gets as far as the missing device -- after every argument check
    assert raw_run(cart, 6, 5, CARTPOLE, rows)[0] == E_DEVICE and "host-only" in cart.error()
    assert raw_run(di, 6, 5, LINEAR, lin2)[0] == E_DEVICE
    refused(reg, 6, 5, CARTPOLE, rows, "regulator handle")
    refused(cart, 0, 5, CARTPOLE, rows, "B >= 1")
    refused(cart, 6, 0, CARTPOLE, rows, "T >= 1")
    refused(cart, -2, 5, CARTPOLE, rows, "B >= 1")
    refused(cart, 6, 5, 2, rows, "kind")                                  # TMPC_PLANT_EXTERNAL is no family
    refused(cart, 6, 5, 7, rows, "kind")
    refused(di, 6, 5, CARTPOLE, rows, "nx = 4, nu = 1")
    refused(cart, 6, 5, CARTPOLE, rows, "substeps >= 1", substeps=0)
    refused(cart, 6, 5, CARTPOLE, None, "models is NULL")
    for kw in (dict(p_loss=None), dict(ref=None), dict(th=None), dict(ga=None), dict(w=None)):
        refused(cart, 6, 5, CARTPOLE, rows, "NULL argument", **kw)
    refused(cart, 6, 5, CARTPOLE, rows, "extended = 1", extended=1)
    # rows that are no plant: the rule and the words of tmpc_estimate_w_models
    for col, name, bad in ((0, "M", 0.0), (1, "m", -1.0), (5, "l", 0.0), (3, "I", -1e-3), (2, "b", -0.1), (6, "Th", 0.0), (4, "g", np.nan), (0, "M", np.inf)):
        r = rows.copy()
        r[2, col] = bad
        refused(cart, 6, 5, CARTPOLE, r, name + " of trajectory 2")
    for (i, j), name in (((1, 0), "A[1, 0] of trajectory 4"), ((0, 2), "B[0, 0] of trajectory 4")):
        for bad in (np.nan, -np.inf):
            m = lin2.copy()
            m[4, i, j] = bad
            refused(di, 6, 5, LINEAR, m, name, "not finite")
    # a reference table and a channel that are set bind the batch; refused calls leave both as they were
    L = _native.lib()
    assert _native.mc_set_channel(cart, montecarlo.burst_channel(np.full(6, 0.3), 3.0)) == 6
    thr = _native.mc_get_channel(cart, 6)
    refused(cart, 4, 5, CARTPOLE, rows[:4], "B = 4, but the loss channel was set for B = 6")
    _native.mc_set_reference(cart, np.zeros((1, 8, 4)), B=6)
    refused(cart, 4, 5, CARTPOLE, rows[:4], "B = 4, but the reference table was set for B = 6")
    refused(cart, 6, 9, CARTPOLE, rows, "T = 9 steps, but the reference table has T_tab = 8 rows")
    assert raw_run(cart, 6, 5, CARTPOLE, rows, p_loss=None, ref=None)[0] == E_DEVICE          # with both set neither p_loss nor ref is read
    assert np.array_equal(_native.mc_get_channel(cart, 6), thr)
    _native.mc_set_reference(cart, None)
    _native.mc_set_channel(cart, None)
    # with the device generator the draws may be NULL
    assert L.tmpc_mc_set_device_rng(cart.ptr, 1, 5, 0, np.zeros(4).ctypes.data) == 0
    assert raw_run(cart, 6, 5, CARTPOLE, rows, th=None, ga=None, w=None)[0] == E_DEVICE
    assert L.tmpc_mc_set_device_rng(cart.ptr, 0, 0, 0, None) == 0
    refused(cart, 6, 5, CARTPOLE, rows, "NULL argument", w=None)
    # the setter of the regulator loop still refuses tracking handles
    assert L.tmpc_mc_set_plant_models(cart.ptr, LINEAR, 6, np.zeros((6, 4, 5)).ctypes.data, 0) == -2 and "only regulator handles" in cart.error()
    # the Python entry points check the family against the batch before the library sees it
    with pytest.raises(ValueError, match="holds 6 plants, the loop 5"):
        _native.mc_run_plants(cart, montecarlo.plant_family("cartpole", par=rows), np.zeros(5), np.zeros(3), np.zeros((5, 3)), np.zeros((5, 3)), np.zeros((5, 3, 4)))
    with pytest.raises(ValueError, match="PlantFamily"):
        _native.mc_run_plants(cart, "cartpole", np.zeros(5), np.zeros(3), np.zeros((5, 3)), np.zeros((5, 3)), np.zeros((5, 3, 4)))


def test_plant_step_refusals_come_before_the_device(hip_lib):
    L = _native.lib()
    buf = np.zeros(4096)                       # never read: every call below is refused on its arguments
    p = buf.ctypes.data

    def refused(*args):
        words = [a for a in args if isinstance(a, str)]
        rc = L.tmpc_plant_step_device(*[a for a in args if not isinstance(a, str)])
        msg = L.tmpc_last_error(None).decode()
        assert rc == E_INVALID and msg.startswith("tmpc_plant_step_device: "), (rc, msg)
        for wd in words:
            assert wd in msg, (wd, msg)

    far = p + 8 * 1024
    refused(0, CARTPOLE, 4, 1, 0, p, 10, p, p, None, far, None, "B < 1")
    refused(0, 2, 4, 1, 8, p, 10, p, p, None, far, None, "kind")
    refused(0, CARTPOLE, 3, 1, 8, p, 10, p, p, None, far, None, "nx = 4, nu = 1")
    refused(0, CARTPOLE, 4, 2, 8, p, 10, p, p, None, far, None, "nx = 4, nu = 1")
    refused(0, CARTPOLE, 4, 1, 8, p, 0, p, p, None, far, None, "substeps >= 1")
    refused(0, LINEAR, 17, 1, 8, p, 0, p, p, None, far, None, "1 <= nx <= 16")
    refused(0, LINEAR, 3, 0, 8, p, 0, p, p, None, far, None, "1 <= nu <= 16")
    for k in range(4):                         # models, x, u, x_plus
        ptrs = [p, p, p, far]
        ptrs[k] = None
        refused(0, LINEAR, 3, 2, 8, ptrs[0], 0, ptrs[1], ptrs[2], None, ptrs[3], None, "NULL")
    # x_plus inside, at and across the ends of x; one past the end is fine for the check (the next refusal is the device's)
    nbytes = 8 * 3 * 8
    for off in (0, 8, nbytes - 8, -8, -(nbytes - 8)):
        refused(0, LINEAR, 3, 2, 8, p, 0, p + 1024, p, None, p + 1024 + off, None, "overlaps x")


# ------------------------------------------------------------------------------------------------ the kernels' source on the host model
@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    """The host-model programs under the sanitizers (tests/wavesim/hostsim.py: a host without their runtimes skips, a program that does not
    build fails).  Stand-alone programs: nothing is loaded into Python under a sanitizer."""
    return hostsim.binaries_or_skip(tmp_path_factory, "plantstep")


def cartpole_inputs(nb, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (nb, 4)) * [1.0, 1.0, 0.3, 1.0], rng.uniform(-10, 10, (nb, 1))


@pytest.mark.parametrize("build", ["plantstep_asan", "plantstep_msan"])
@pytest.mark.parametrize("nb", [1, 65])
def test_cartpole_kernel_on_the_host_model(binaries, build, nb):
    """Spread-0.2 cart-poles, one lane each (65: a full wave and a workgroup of one lane), one trajectory held; w from an array, from the
    device generator and absent; the physics-rate error against the legacy reference and against a table row."""
    fam = montecarlo.sample_cartpole(nb, 0.2, 5)
    x, u = cartpole_inputs(nb, 1)
    want = fam(x, u)
    held = nb // 2
    hold = np.zeros(nb, dtype=np.uint8)
    hold[held] = 1
    w_bound = np.array([1e-3, 2e-3, 3e-3, 4e-3])
    t, seed, first = 7, 99, 12
    _, _, wp = montecarlo.draw_realisations_philox(nb, t + 1, w_bound, seed=seed, first=first)
    w_arr = np.random.default_rng(2).uniform(-1e-2, 1e-2, (nb, 4))
    for kw, w in ((dict(), None), (dict(w=w_arr), w_arr), (dict(philox=(t, seed, first, w_bound)), wp[:, t])):
        out = plantstep_case.run_step(binaries[build], fam, x, u, hold=hold, env=hostsim.SAN_ENV, **kw)
        hostsim.assert_clean(out["stderr"])
        exp = want if w is None else want + w
        exp[held] = x[held]
        np.testing.assert_allclose(out["x_plus"], exp, atol=CARTPOLE_ATOL, rtol=0)
        assert np.array_equal(out["x_plus"][held], x[held])
    # the physics-rate error: the sum over the states at the start of every physics step, added to what the accumulator held
    tr = fam.trace(x, u)[:-1]                                            # (substeps, B, 4)
    before = np.arange(nb, dtype=np.float64)
    tab = np.random.default_rng(3).uniform(-0.5, 0.5, (2, t + 2, 4))
    ids = np.arange(nb) % 2
    for kw, r in ((dict(ref_t=0.4), np.tile([0.4, 0.0, 0.0, 0.0], (nb, 1))), (dict(ref_tab=tab, ref_id=ids, philox=(t, 0, 0, None)), tab[ids, t])):
        out = plantstep_case.run_step(binaries[build], fam, x, u, hold=hold, err2_phys=before, env=hostsim.SAN_ENV, **kw)
        hostsim.assert_clean(out["stderr"])
        exp = before + ((tr - r[None]) ** 2).sum(axis=(0, 2))
        live = hold == 0
        # every state behind the sum is the twin's within CARTPOLE_ATOL, so the sum of the (y - r)^2 moves by at most 2 atol sum |y - r| (+ atol^2
        # terms, far below); the 4 substeps + 1 additions round within (4 substeps + 1) eps of the result
        bound = 2.0 * CARTPOLE_ATOL * np.abs(tr - r[None]).sum(axis=(0, 2)) + (4 * fam.substeps + 1) * EPS * np.abs(exp)
        assert np.all(np.abs(out["err2_phys"][live] - exp[live]) <= bound[live]), float(np.max(np.abs(out["err2_phys"][live] - exp[live]) / bound[live]))
        assert np.isnan(out["err2_phys"][held])                           # tmpc_mc_get_physics_error: NaN for a trajectory that stopped


@pytest.mark.parametrize("build", ["plantstep_asan", "plantstep_msan"])
@pytest.mark.parametrize("nx,nu", [(1, 1), (3, 2), (16, 4)])
def test_linear_kernel_on_the_host_model(binaries, build, nx, nu):
    """One lane per (trajectory, state row), B = 5: w from an array, from the device generator and absent, against the numpy twin within
    the bound of the sum; a held trajectory keeps its state; a zero model returns the generator's w, which must be the host twin's bytes."""
    nb = 5
    fam = linear_family(nb, nx, nu, 10 * nx + nu)
    rng = np.random.default_rng(4)
    x, u = rng.uniform(-2, 2, (nb, nx)), rng.uniform(-2, 2, (nb, nu))
    w_bound = np.linspace(1e-3, 5e-2, nx)
    t, seed, first = 3, 2024, 40
    _, _, wp = montecarlo.draw_realisations_philox(nb, t + 1, w_bound, seed=seed, first=first)
    w_arr = rng.uniform(-0.1, 0.1, (nb, nx))
    hold = np.zeros(nb, dtype=np.uint8)
    hold[3] = 1
    for kw, w in ((dict(), None), (dict(w=w_arr), w_arr), (dict(philox=(t, seed, first, w_bound)), wp[:, t])):
        for hd in (None, hold):
            out = plantstep_case.run_step(binaries[build], fam, x, u, hold=hd, env=hostsim.SAN_ENV, **kw)
            hostsim.assert_clean(out["stderr"])
            exp = fam(x, u) if w is None else fam(x, u) + w
            bound = linear_bound(fam, x, u, w)
            if hd is not None:
                exp[3], bound[3] = x[3], 0.0
            assert np.all(np.abs(out["x_plus"] - exp) <= bound), float(np.max(np.abs(out["x_plus"] - exp) - bound))
    zero = montecarlo.plant_family("linear", A=np.zeros((nb, nx, nx)), B=np.zeros((nb, nx, nu)))
    out = plantstep_case.run_step(binaries[build], zero, x, u, philox=(t, seed, first, w_bound), env=hostsim.SAN_ENV)
    hostsim.assert_clean(out["stderr"])
    assert out["x_plus"].tobytes() == np.ascontiguousarray(wp[:, t]).tobytes()


def test_plant_kernels_have_no_private_segment_and_no_lds():
    """The cart-pole lane keeps its seven parameters, four states and the RK4 stages in registers; neither kernel uses LDS."""
    from test_code_objects import _kernels
    ks = {n: k for n, k in _kernels().items() if "plant_cartpole_kernel" in n or "plant_linear_kernel" in n}
    assert len(ks) == 2, sorted(ks)
    for n, k in ks.items():
        assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".group_segment_fixed_size"] == 0, (n, k)
