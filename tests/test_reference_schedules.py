"""Full-state reference schedules per trajectory in the closed loops (include/tmpc.h: tmpc_mc_set_reference_table; the (T, nx),
(B, T, nx) and (K, T, nx) + ref_id forms of `ref` in TubeTrackingMPC.run_closed_loop and the (B, T, nx) form of the host twins in
montecarlo).  Without a GPU: the setter's validation on host-only handles and the host twins with the oracle as the solver.  On the
GPU: the legacy reference restated as a table gives the legacy bytes in every loop form; the device loop against the host loop
within the project's bands for that comparison (tests/test_closed_loop_several_inputs.py: _compare); fused against per-step and
one call against two half calls, bytes."""
import ctypes as C

import numpy as np
import pytest

import common
import regulator_problems as rp
from LinearMPCOverNetworks import _native, montecarlo
from oracle.oracle import Oracle
from test_closed_loop import _oracle_packets
from test_closed_loop_several_inputs import KEYS, _compare, two_input_mpc

E_INVALID = -1                                         # include/tmpc.h
P_LOSS = np.tile([0.0, 0.3, 0.6, 0.9], 4)              # B = 16
NB = 16


# ------------------------------------------------------------------------------------------------ the tables
def cartpole_table(T=24):
    """K = 4 schedules that are no steady states: a step, a moving cart, a sine with a tilted pole, a swinging set-point."""
    t = np.arange(T)
    tab = np.zeros((4, T, 4))
    tab[0, :, 0] = np.where(t < T // 2, 0.5, -0.3)
    tab[1, :, 0], tab[1, :, 1] = 0.4, 0.2
    tab[2, :, 0], tab[2, :, 2] = -0.5 * np.sin(t / 4.0), 0.05
    tab[3, :, 0], tab[3, :, 3] = 0.3, 0.1 * (-1.0) ** (t // 3)
    return tab, ((np.arange(NB) * 7 + 1) % 4).astype(np.int32)


def two_input_table(T=12, nb=NB):
    t = np.arange(T)
    tab = np.zeros((3, T, 3))
    tab[0, :, 0] = np.where(t < T // 2, 2.0, -1.2)
    tab[1] = [1.0, -0.5, 0.8]
    tab[2, :, 1], tab[2, :, 2] = 1.5 * (-1.0) ** (t // 2), -1.0
    return tab, ((np.arange(nb) * 5 + 2) % 3).astype(np.int32)


def config5_table(T=12):
    """nx = 12: set-points in the states 0, 2, 4, 6, 9 and 11 (four of them beyond the fourth), one schedule per trajectory pair."""
    t = np.arange(T)
    tab = np.zeros((8, T, 12))
    for k in range(8):
        tab[k, :, 0] = np.where(t < T // 2, 0.2, -0.1) * (1 + k % 3)
        tab[k, :, 2] = 0.05 * (k - 3)
        tab[k, :, 4] = 0.1 * np.sin(t / 3.0 + k)
        tab[k, :, 6] = -0.08 + 0.02 * k
        tab[k, :, 9] = 0.06 * (-1.0) ** (t // 4)
        tab[k, :, 11] = 0.03 * k
    return tab, (np.arange(NB) // 2).astype(np.int32)


def legacy_as_table(ref, nx):
    """(T,) -> (T, nx): [ref_t, 0, .., 0]"""
    tab = np.zeros((len(ref), nx))
    tab[:, 0] = ref
    return tab


def host_loop(mpc, w, packets, p_loss, ref, th, ga, dist, extended, **kw):
    return montecarlo.run_remote_tube_mpc(packets, w["A"], w["B"], mpc.get_steady_state_controller_gain(),
                                          mpc.get_ancillary_controller_gain(), mpc._N, mpc._Z, p_loss, ref, th, ga, dist,
                                          extended=extended, **kw)


# ------------------------------------------------------------------------------------------------ CPU 1: the setter
@pytest.fixture(scope="module")
def host_handle(hip_lib):
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True, device=-1)
    yield mpc._handle
    mpc._close()


def _set(h, K, T_tab, table, B, ids):
    tab, ids = [None if a is None else np.ascontiguousarray(a, dtype=d) for a, d in ((table, np.float64), (ids, np.int32))]
    rc = _native.lib().tmpc_mc_set_reference_table(h.ptr, K, T_tab, None if tab is None else tab.ctypes.data, B,
                                                   None if ids is None else ids.ctypes.data)
    return rc, h.error()


def test_exports_and_abi_version(hip_lib):
    L = _native.lib()
    for name, nargs in (("tmpc_mc_set_reference_table", 6), ("tmpc_mc_step_device_ref", 5), ("tmpc_mc_step_ref", 4)):
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == nargs, name
    assert L.tmpc_abi_version() == _native.ABI_VERSION == 5
    assert "#define TMPC_ABI_VERSION 5" in open(common.ROOT + "/include/tmpc.h").read()
    assert L.tmpc_mc_set_reference_table(None, 1, 1, None, 1, None) == E_INVALID


def test_setter_accepts_the_forms_on_a_host_only_handle(host_handle):
    h = host_handle
    tab = np.arange(3 * 5 * 4, dtype=np.float64).reshape(3, 5, 4)
    assert _set(h, 1, 5, tab[:1], 7, None)[0] == 0                       # K == 1, ref_id NULL: schedule 0 for everybody
    assert _set(h, 3, 5, tab, 3, None)[0] == 0                           # K == B, ref_id NULL: schedule b
    assert _set(h, 3, 5, tab, 6, [0, 2, 1, 1, 0, 2])[0] == 0
    assert _set(h, 0, 0, None, 0, None)[0] == 0                          # clear
    assert _set(h, 0, -4, None, -1, None)[0] == 0                        # (K == 0: the other arguments are ignored)
    _native.mc_set_reference(h, tab, [2, 0])                             # the binding
    _native.mc_set_reference(h, tab[0])
    _native.mc_set_reference(h, None)


def test_binding_tells_the_reference_forms_apart(host_handle):
    h, nx = host_handle, 4
    f = _native._loop_reference
    leg, T = f(h, "t", np.arange(6.0), 3, None, None)
    assert leg.shape == (6,) and T == 6
    assert f(h, "t", np.arange(4.0), 3, 4, None)[0].shape == (4,)            # (nx,) with T <= nx stays the legacy form
    assert f(h, "t", np.arange(4.0), 3, 9, None) == (None, 9)                # (nx,) with T > nx: constant
    assert f(h, "t", np.arange(4.0)[None], 3, 2, None) == (None, 2)          # (1, nx): constant for every T
    assert f(h, "t", np.zeros((7, nx)), 3, None, None) == (None, 7)
    assert f(h, "t", np.zeros((3, 7, nx)), 3, None, None) == (None, 7)
    assert f(h, "t", np.zeros((2, 7, nx)), 3, 5, [0, 1, 1]) == (None, 5)
    with pytest.raises(ValueError, match="no ref_id"):
        f(h, "t", np.zeros((2, 7, nx)), 3, None, None)
    with pytest.raises(ValueError, match="nx = 4"):
        f(h, "t", np.zeros((7, nx + 1)), 3, None, None)
    # mc_open has always flattened its legacy reference: a scalar, a row, a column
    for ref, n in ((0.5, 1), (np.zeros((1, 6)), 6), (np.zeros((6, 1)), 6)):
        leg, T = f(h, "t", ref, 3, None, None, flatten_legacy=True)
        assert leg.shape == (n,) and T == n
    _native.mc_set_reference(h, None)


@pytest.mark.parametrize("label,args", [
    ("K < 0", (-1, 5, True, 3, None)),
    ("T_tab < 1", (3, 0, True, 3, None)),
    ("B < 1", (3, 5, True, 0, None)),
    ("no table", (3, 5, None, 3, None)),
    ("no ids, K neither 1 nor B", (3, 5, True, 4, None)),
    ("id too large", (3, 5, True, 4, [0, 1, 3, 2])),
    ("negative id", (3, 5, True, 4, [0, -1, 2, 2])),
])
def test_setter_rejects_with_a_message(host_handle, label, args):
    K, T_tab, table, B, ids = args
    if table is True:
        table = np.zeros((max(K, 1), max(T_tab, 1), 4))
    rc, msg = _set(host_handle, K, T_tab, table, B, ids)
    assert rc == E_INVALID and msg.startswith("tmpc_mc_set_reference_table: "), (label, rc, msg)


def test_setter_refuses_a_regulator_handle(hip_lib):
    m = rp.plain_double_integrator(device=-1)
    try:
        rc, msg = _set(m._handle, 1, 5, np.zeros((1, 5, 2)), 3, None)
        assert rc == E_INVALID and "regulator" in msg
    finally:
        m._close()


# ------------------------------------------------------------------------------------------------ CPU 2: the host twins
def _cpu_case(name, extended):
    if name == "cartpole":
        mpc, w = common.make_mpc("cartpole", 10, True, extended=extended)
        tab, ids = cartpole_table()
        seed = 11
    elif name == "two_input":
        mpc, w = two_input_mpc(extended, device=-1)
        tab, ids = two_input_table()
        seed = 32
    else:
        mpc, w = common.make_mpc("synthetic", 30, True)
        tab, ids = config5_table()
        seed = 55
    th, ga, dist = montecarlo.draw_realisations(NB, tab.shape[1], w["w_bound"], seed=seed)
    return mpc, w, tab, ids, th, ga, dist


@pytest.mark.parametrize("extended", [False, True])
def test_host_twin_legacy_reference_as_full_states_bit_for_bit(oracle_lib, extended):
    mpc, w, _, _, th, ga, dist = _cpu_case("cartpole", extended)
    T = th.shape[1]
    ref = np.where(np.arange(T) < T // 2, 0.5, -0.3)
    full = np.broadcast_to(legacy_as_table(ref, 4), (NB, T, 4))
    pk = _oracle_packets(mpc, Oracle(mpc._problem_dict()))
    a = host_loop(mpc, w, pk, P_LOSS, ref, th, ga, dist, extended, capture=7)
    b = host_loop(mpc, w, pk, P_LOSS, full, th, ga, dist, extended, capture=7)
    for k in ("tracking_error", "tube_violations", "not_optimal", "x_final", "x_traj", "x_nom_traj", "u_traj"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


@pytest.mark.parametrize("name,extended", [("cartpole", False), ("cartpole", True), ("two_input", False), ("two_input", True),
                                           ("config5", False)])
def test_host_twin_tracks_the_tables(oracle_lib, name, extended):
    """The condition on the inputs of the GPU comparisons: with these tables every solve is OPTIMAL and the tube holds."""
    mpc, w, tab, ids, th, ga, dist = _cpu_case(name, extended)
    try:
        out = host_loop(mpc, w, _oracle_packets(mpc, Oracle(mpc._problem_dict())), P_LOSS, tab[ids], th, ga, dist, extended)
        assert np.all(out["not_optimal"] == 0) and np.all(out["tube_violations"] == 0)
        assert np.all(np.isfinite(out["tracking_error"])) and out["tracking_error"].max() > 0
        # the error statistic is against the full state: a schedule with a set-point in a later state scores differently
        # from the legacy statistic of its first column
        leg = host_loop(mpc, w, _oracle_packets(mpc, Oracle(mpc._problem_dict())), P_LOSS, tab[ids][:, :, 0], th, ga, dist, extended)
        assert np.max(np.abs(leg["tracking_error"] - out["tracking_error"])) > 1e-3
    finally:
        mpc._close()


def test_rmpc_host_twin_runs_the_cartpole_table(oracle_lib):
    from test_tracking_mpc import _bare
    mpc, w = _bare("cartpole", 10)
    tab, ids = cartpole_table()
    T = tab.shape[1]
    th, ga, dist = montecarlo.draw_realisations(NB, T, w["w_bound"], seed=11)
    pk = _oracle_packets(mpc, Oracle(mpc._problem_dict()))
    K = mpc.get_steady_state_controller_gain()
    out = montecarlo.run_remote_tracking_mpc(pk, w["A"], w["B"], K, 10, P_LOSS, tab[ids], th, ga, dist)
    alive = ~out["infeasible"]
    assert alive.any() and np.all(np.isfinite(out["tracking_error"][alive])) and np.all(np.isnan(out["tracking_error"][~alive]))
    ref = tab[0, :, 0]
    a = montecarlo.run_remote_tracking_mpc(pk, w["A"], w["B"], K, 10, P_LOSS, ref, th, ga, dist)
    b = montecarlo.run_remote_tracking_mpc(pk, w["A"], w["B"], K, 10, P_LOSS, np.broadcast_to(legacy_as_table(ref, 4), (NB, T, 4)),
                                           th, ga, dist)
    for k in ("tracking_error", "not_optimal", "infeasible", "x_final"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


# ------------------------------------------------------------------------------------------------ CPU 3: shards of the host sweep
class _OracleController:
    """What montecarlo.mc_sweep's host branch asks of a controller, answered by the oracle."""

    def __init__(self, mpc):
        self._mpc, self._N, self._Z = mpc, mpc._N, mpc._Z
        self.determine_packets = _oracle_packets(mpc, Oracle(mpc._problem_dict()))
        self.get_steady_state_controller_gain = mpc.get_steady_state_controller_gain
        self.get_ancillary_controller_gain = mpc.get_ancillary_controller_gain


def test_host_sweep_with_reference_ids_is_shard_invariant(oracle_lib, monkeypatch):
    mpc, w = two_input_mpc(False, device=-1)
    monkeypatch.setattr(montecarlo, "gather_statistics", lambda local, *a, **k: local)      # each rank's own rows, no process group
    try:
        tab, _ = two_input_table()
        p_loss, n_mc, T = np.array([0.0, 0.3, 0.6, 0.9]), 3, tab.shape[1]
        ids = (np.arange(12) * 5 + 2) % 3
        ctl = _OracleController(mpc)
        one, pi = montecarlo.mc_sweep(ctl, w, p_loss, n_mc, T, tab, seed=32, ref_id=ids)
        parts = [montecarlo.mc_sweep(ctl, w, p_loss, n_mc, T, tab, seed=32, ref_id=ids, rank=r, world=2)[0] for r in range(2)]
        assert one.shape == (12, 3) and np.all(one[:, 2] == 0) and [len(p) for p in parts] == [6, 6]
        assert np.concatenate(parts).tobytes() == one.tobytes()
        other = montecarlo.mc_sweep(ctl, w, p_loss, n_mc, T, tab, seed=32, ref_id=(ids + 1) % 3)[0]
        assert np.max(np.abs(other[:, 0] - one[:, 0])) > 1e-3                 # the ids matter
    finally:
        mpc._close()


# ------------------------------------------------------------------------------------------------ GPU
_MPC = {}


def _cartpole(extended):
    if extended not in _MPC:
        _MPC[extended] = common.make_mpc("cartpole", 10, True, extended=extended, create=True)
    return _MPC[extended]


def _same_bytes(a, b, keys):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (k, np.asarray(a[k]), np.asarray(b[k]))


# -- 4: the legacy reference as a table, byte for byte
@pytest.mark.gpu
@pytest.mark.parametrize("extended,fused,mode", [(False, "on", 1), (False, "off", 0), (True, "on", 2), (True, "off", 0)])
def test_table_of_the_legacy_reference_gives_the_legacy_bytes(hip_lib, extended, fused, mode):
    mpc, w = _cartpole(extended)
    T = 24
    ref = np.where(np.arange(T) < T // 2, 0.5, -0.3)
    th, ga, dist = montecarlo.draw_realisations(NB, T, w["w_bound"], seed=11)
    kw = dict(extended=extended, capture=7, fused=fused)
    leg = mpc.run_closed_loop(P_LOSS, ref, th, ga, dist, **kw)
    tab = mpc.run_closed_loop(P_LOSS, legacy_as_table(ref, 4), th, ga, dist, **kw)
    assert leg["loop_mode"] == tab["loop_mode"] == mode
    _same_bytes(tab, leg, KEYS)
    assert np.all(leg["not_optimal"] == 0) and leg["err2"].min() > 0
    again = mpc.run_closed_loop(P_LOSS, ref, th, ga, dist, **kw)            # a (T,) call clears the table
    _same_bytes(again, leg, KEYS)


@pytest.mark.gpu
def test_table_of_the_legacy_reference_rmpc_with_a_trajectory_that_stops(hip_lib):
    from test_tracking_mpc import _make
    mpc, w = _make(True)
    try:
        nb, T = 64, 24
        x0 = np.random.default_rng(11).uniform(-1, 1, (nb, 2)) * [7.6, 0.6]
        p_loss = np.tile([0.0, 0.3, 0.6, 0.9], nb // 4)
        th, ga, dist = montecarlo.draw_realisations(nb, T, 3.0 * w["w_bound"], seed=5)
        ref = np.where(np.arange(T) < T // 2, 6.0, -6.0)
        for fused in ("on", "off"):
            leg = mpc.run_closed_loop(p_loss, ref, th, ga, dist, x0=x0, capture=3, fused=fused)
            tab = mpc.run_closed_loop(p_loss, legacy_as_table(ref, 2), th, ga, dist, x0=x0, capture=3, fused=fused)
            dead = np.isnan(leg["tracking_error"])
            assert 0 < dead.sum() < nb
            _same_bytes(tab, leg, KEYS)
    finally:
        mpc._close()


@pytest.mark.gpu
def test_table_of_the_legacy_reference_cartpole_plant_and_block_path(hip_lib):
    mpc, w = _cartpole(False)
    T = 24
    ref = np.where(np.arange(T) < T // 2, 0.5, -0.3)
    th, ga, dist = montecarlo.draw_realisations(NB, T, w["w_bound"], seed=11)
    for fused in ("on", "off"):
        leg = mpc.run_closed_loop(P_LOSS, ref, th, ga, 0.0 * dist, plant="cartpole", capture=7, fused=fused)
        tab = mpc.run_closed_loop(P_LOSS, legacy_as_table(ref, 4), th, ga, 0.0 * dist, plant="cartpole", capture=7, fused=fused)
        _same_bytes(tab, leg, KEYS + ("err2_physics", "tracking_error_physics"))
        assert leg["err2_physics"].min() > 0
    try:
        mpc.set_kernel_path("block")
        leg = mpc.run_closed_loop(P_LOSS, ref, th, ga, dist, capture=7)
        tab = mpc.run_closed_loop(P_LOSS, legacy_as_table(ref, 4), th, ga, dist, capture=7)
        assert leg["loop_mode"] == tab["loop_mode"] == 0 and mpc.get_kernel_path() == "block"
        _same_bytes(tab, leg, KEYS)
    finally:
        mpc.set_kernel_path("auto")


# -- 5: the device loop against the host loop around the same handle's solves
def _device_vs_host(label, mpc, w, tab, ids, extended, seed):
    T = tab.shape[1]
    full = tab[ids]
    th, ga, dist = montecarlo.draw_realisations(NB, T, w["w_bound"], seed=seed)
    host = host_loop(mpc, w, mpc.determine_packets, P_LOSS, full, th, ga, dist, extended, capture=7)
    dev = mpc.run_closed_loop(P_LOSS, tab, th, ga, dist, extended=extended, capture=7, ref_id=ids)
    _compare(label + ", host draws", dev, host)
    per = mpc.run_closed_loop(P_LOSS, full, th, ga, dist, extended=extended, capture=7)         # (B, T, nx): the same numbers
    _same_bytes(per, dev, KEYS)
    thp, gap, distp = montecarlo.draw_realisations_philox(NB, T, w["w_bound"], seed=seed, first=500)
    host = host_loop(mpc, w, mpc.determine_packets, P_LOSS, full, thp, gap, distp, extended, capture=7)
    dev = mpc.run_closed_loop(P_LOSS, tab, extended=extended, capture=7, device_rng=(seed, 500, w["w_bound"]), ref_id=ids)
    _compare(label + ", device generator", dev, host)


@pytest.mark.gpu
@pytest.mark.parametrize("extended", [False, True])
def test_cartpole_device_loop_equals_host_loop_with_schedules(hip_lib, extended):
    mpc, w = _cartpole(extended)
    _device_vs_host(f"cart-pole N 10, 4 schedules, extended = {extended}", mpc, w, *cartpole_table(), extended, seed=11)


@pytest.mark.gpu
@pytest.mark.parametrize("extended", [False, True])
def test_two_input_device_loop_equals_host_loop_with_schedules(hip_lib, extended):
    mpc, w = two_input_mpc(extended, device=0)
    try:
        _device_vs_host(f"two inputs, 3 schedules, extended = {extended}", mpc, w, *two_input_table(), extended, seed=32)
    finally:
        mpc._close()


@pytest.mark.gpu
def test_config5_device_loop_equals_host_loop_with_schedules(hip_lib):
    mpc, w = common.make_mpc("synthetic", 30, True, create=True)
    try:
        assert (mpc._nx, mpc._nu) == (12, 4) and mpc.get_kernel_path() == "block"
        _device_vs_host("config 5 (nx 12, nu 4, N 30), block kernel, 8 schedules", mpc, w, *config5_table(), False, seed=55)
    finally:
        mpc._close()


# -- 6: fused against the launch pair per step
@pytest.mark.gpu
@pytest.mark.parametrize("extended,warm", [(False, False), (False, True), (True, False), (True, True)])
def test_fused_loops_equal_the_launch_pair_per_step_with_schedules(hip_lib, extended, warm):
    mpc, w = two_input_mpc(extended, device=0)
    try:
        nb, steps = 40, 16
        tab, ids = two_input_table(steps, nb)
        p_loss = np.tile(np.arange(10) / 10.0, nb // 10)
        th, ga, dist = montecarlo.draw_realisations(nb, steps, w["w_bound"], seed=46)
        kw = dict(extended=extended, warm_start=warm, capture=3, ref_id=ids)
        off = mpc.run_closed_loop(p_loss, tab, th, ga, dist, fused="off", **kw)
        on = mpc.run_closed_loop(p_loss, tab, th, ga, dist, fused="on", **kw)
        assert off["loop_mode"] == 0 and on["loop_mode"] == (2 if extended else 1)
        _same_bytes(on, off, KEYS)
        assert np.all(on["not_optimal"] == 0) and np.abs(on["u_traj"]).max() > 1e-3
    finally:
        mpc._close()


# -- 7: one call against two half calls
@pytest.mark.gpu
def test_split_batch_with_sliced_ids_gives_the_same_bytes(hip_lib):
    mpc, w = two_input_mpc(False, device=0)
    try:
        nb, T = 32, 12
        tab, ids = two_input_table(T, nb)
        p_loss = np.tile([0.0, 0.3, 0.6, 0.9], nb // 4)
        keys = ("err2", "tube_violations", "not_optimal", "x_final", "consistent", "iters_sum")
        one = mpc.run_closed_loop(p_loss, tab, device_rng=(32, 100, w["w_bound"]), ref_id=ids)
        halves = [mpc.run_closed_loop(p_loss[lo:lo + 16], tab, device_rng=(32, 100 + lo, w["w_bound"]), ref_id=ids[lo:lo + 16])
                  for lo in (0, 16)]
        for k in keys:
            assert np.concatenate([h[k] for h in halves]).tobytes() == one[k].tobytes(), k
        assert np.all(one["not_optimal"] == 0)
    finally:
        mpc._close()
