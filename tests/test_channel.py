"""The Gilbert-Elliott loss channel and the link statistics without a GPU (include/tmpc.h: tmpc_mc_set_channel / _get_channel /
_get_link_stats): the host arithmetic of the thresholds against its numpy twin bit for bit, the twin's flags in its degenerate
cases and in distribution, the argument errors of the exports, and the link statistics of the host loops on a hand-written
pattern."""
import ctypes as C

import numpy as np
import pytest

import common
import regulator_problems as rp
from LinearMPCOverNetworks import _native, montecarlo, workloads
from LinearMPCOverNetworks.polytope_lite import Polytope

E_INVALID = -1                                         # include/tmpc.h


@pytest.fixture(scope="module")
def host_handle(hip_lib):
    mpc, _ = common.make_mpc("cartpole", 10, True, create=True, device=-1)
    yield mpc._handle
    mpc._close()


def _set(h, B, *par):
    keep = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in par]
    rc = _native.lib().tmpc_mc_set_channel(h.ptr, B, *[None if a is None else a.ctypes.data for a in keep])
    return rc, h.error()


# ------------------------------------------------------------------------------------------------ the thresholds
def test_exports_exist_and_are_bound(hip_lib):
    L = _native.lib()
    for name, nargs in (("tmpc_mc_set_channel", 6), ("tmpc_mc_get_channel", 3), ("tmpc_mc_get_link_stats", 6)):
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == nargs, name
    for name in ("mc_set_channel", "mc_get_channel", "mc_link_stats"):
        assert callable(getattr(_native, name))
    for name in ("gilbert_elliott_thresholds", "channel_arrivals", "burst_channel"):
        assert callable(getattr(montecarlo, name))
    assert L.tmpc_mc_set_channel(None, 0, None, None, None, None) == E_INVALID
    assert _native.ABI_VERSION == L.tmpc_abi_version() == 5                    # added without a bump


def test_host_thresholds_equal_the_numpy_twin_bit_for_bit(host_handle):
    rng = np.random.default_rng(3)
    edge = np.array([0.0, 1.0])
    grid = np.array(np.meshgrid(edge, edge, edge, edge)).reshape(4, -1)          # every combination of the edge values
    par = np.concatenate([rng.uniform(size=(4, 500)), grid, np.where(rng.uniform(size=(4, 100)) < 0.5, rng.uniform(size=(4, 100)), grid[:, :1])], axis=1)
    B = par.shape[1]
    _native.mc_set_channel(host_handle, tuple(par))
    try:
        got = _native.mc_get_channel(host_handle, B)
        want = montecarlo.gilbert_elliott_thresholds(*par)
        assert got.shape == want.shape == (B, 2, 3)
        assert got.tobytes() == want.tobytes()
        # written out once more, independently of the twin: a = p_gb | 1 - p_bg; [a e_b, a, a + (1 - a) e_g], each operation rounded
        for prev, a in ((0, par[0]), (1, 1.0 - par[1])):
            assert np.array_equal(got[:, prev, 0], a * par[3]) and np.array_equal(got[:, prev, 1], a)
            assert np.array_equal(got[:, prev, 2], a + (1.0 - a) * par[2])
        assert np.all(got[:, :, 0] <= got[:, :, 1]) and np.all(got[:, :, 1] <= got[:, :, 2]) and np.all(got[:, :, 2] <= 1.0)
        assert _native.lib().tmpc_mc_get_channel(host_handle.ptr, B + 1, got.ctypes.data) == E_INVALID
    finally:
        _native.mc_set_channel(host_handle, None)
    assert _native.lib().tmpc_mc_get_channel(host_handle.ptr, B, got.ctypes.data) == E_INVALID      # cleared


def test_degenerate_channel_has_the_bernoulli_thresholds(host_handle):
    p = np.r_[np.random.default_rng(4).uniform(size=64), 0.0, 1.0, 0.3, 0.9]
    B = p.size
    _native.mc_set_channel(host_handle, dict(p_gb=0.0, p_bg=0.37, e_g=p, e_b=0.8), B=B)
    try:
        thr = _native.mc_get_channel(host_handle, B)
    finally:
        _native.mc_set_channel(host_handle, None)
    assert np.array_equal(thr[:, 0, 0], np.zeros(B)) and np.array_equal(thr[:, 0, 1], np.zeros(B))
    assert thr[:, 0, 2].tobytes() == p.tobytes()                               # exactly (0, 0, p) after G, and B is never entered
    assert np.array_equal(montecarlo.gilbert_elliott_thresholds(0.0, 0.37, p, 0.8)[:, 0], thr[:, 0])


# ------------------------------------------------------------------------------------------------ the twin's flags
def test_twin_degenerate_and_all_lost_channels():
    rng = np.random.default_rng(5)
    B, T = 33, 50
    th, ga = rng.uniform(size=(B, T)), rng.uniform(size=(B, T))
    p = rng.uniform(size=B)
    p[:3] = [0.0, 1.0, 0.5]
    th[2, 7] = 0.5                                                              # u == p: strict <, the packet arrives
    arr = montecarlo.channel_arrivals(dict(p_gb=0.0, p_bg=0.2, e_g=p, e_b=1.0), th, ga)
    for flags, u in ((arr["theta"], th), (arr["gamma"], ga)):
        want = (u >= p[:, None]).astype(np.uint8)
        want[:, 0] = 1
        assert np.array_equal(flags, want)
    assert arr["theta"][2, 7] == 1
    assert not arr["state_up"].any() and not arr["state_down"].any()
    lost = montecarlo.channel_arrivals(dict(p_gb=1.0, p_bg=0.0, e_g=0.0, e_b=1.0), th, ga)
    assert np.all(lost["theta"][:, 0] == 1) and np.all(lost["gamma"][:, 0] == 1)
    assert not lost["theta"][:, 1:].any() and not lost["gamma"][:, 1:].any()
    assert np.all(lost["state_up"][:, 1:] == 1) and np.all(lost["state_up"][:, 0] == 0)
    # a few trajectories take the twin's scalar loop: the same flags and states as in the batch
    mixed = dict(p_gb=rng.uniform(size=B), p_bg=rng.uniform(size=B), e_g=rng.uniform(size=B), e_b=rng.uniform(size=B))
    full = montecarlo.channel_arrivals(mixed, th, ga)
    assert full["state_up"].any() and not full["state_up"].all() and not full["theta"].all()
    for b in (0, 5, 32):
        one = montecarlo.channel_arrivals({k: v[b:b + 1] for k, v in mixed.items()}, th[b:b + 1], ga[b:b + 1])
        assert all(np.array_equal(one[k][0], full[k][b]) for k in full)
    never = montecarlo.channel_arrivals((0.5, 0.5, 0.0, 0.0), th, ga)
    assert never["theta"].all() and never["gamma"].all() and never["state_up"].any()


def _se_of_mean(x, max_lag):
    """Standard error of the mean of a stationary series from its own autocovariances c_k up to max_lag:
    sqrt((c_0 + 2 sum_k c_k) / n)."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.size, x - x.mean()
    c = np.array([np.dot(d[:n - k], d[k:]) / n for k in range(max_lag + 1)])
    return float(np.sqrt((c[0] + 2.0 * c[1:].sum()) / n)), c / c[0]


def test_burst_channel_has_its_loss_rate_and_burst_length_in_distribution():
    """One chain of 250 000 steps of burst_channel(0.3, 4), seed 2024.  Its loss indicator is a two-state Markov chain whose
    autocorrelation decays like (1 - p_gb - p_bg)^k = 0.643^k (below 1e-9 after 50 lags): the standard error of the loss rate is taken
    from the chain's own autocovariances up to lag 100, sqrt((c_0 + 2 sum c_k) / n) -- about 2.0e-3, against 9.2e-4 for independent
    draws.  The burst lengths are sojourn times (independent, geometric): the same estimator over the sequence of bursts, lags up
    to 20, gives about 2.5e-2.  Both figures are printed."""
    T = 250_000
    ch = montecarlo.burst_channel(0.3, 4.0)
    assert np.allclose(ch["p_bg"], 0.25) and np.allclose(ch["p_gb"] / (ch["p_gb"] + ch["p_bg"]), 0.3)
    assert np.all(ch["e_g"] == 0.0) and np.all(ch["e_b"] == 1.0)
    u = np.random.default_rng(2024).uniform(size=(1, T))
    arr = montecarlo.channel_arrivals(ch, u, u)
    lost = 1 - arr["theta"][0, 1:].astype(np.int64)
    assert np.array_equal(lost, arr["state_up"][0, 1:])                         # the simple Gilbert channel: lost iff in B
    se_rate, rho = _se_of_mean(lost, 100)
    edges = np.flatnonzero(np.diff(np.r_[0, lost, 0]))
    bursts = (edges[1::2] - edges[0::2])[1:-1]                                  # (without the possibly cut first and last burst)
    se_burst, _ = _se_of_mean(bursts, 20)
    print(f"   loss rate {lost.mean():.5f} +- {se_rate:.1e} (lag-1 autocorrelation {rho[1]:.3f}), "
          f"mean burst {bursts.mean():.4f} +- {se_burst:.1e} over {bursts.size} bursts")
    assert abs(rho[1] - (1.0 - 0.25 - ch["p_gb"][0])) < 0.01
    assert 1e-3 < se_rate < 4e-3 and 1e-2 < se_burst < 5e-2
    assert abs(lost.mean() - 0.3) <= 5.0 * se_rate
    assert abs(bursts.mean() - 4.0) <= 5.0 * se_burst


# ------------------------------------------------------------------------------------------------ argument errors
def test_setter_refuses_a_regulator_handle(hip_lib):
    m = rp.plain_double_integrator(device=-1)
    try:
        rc, msg = _set(m._handle, 2, [0.1, 0.1], [0.5, 0.5], [0.0, 0.0], [1.0, 1.0])
        assert rc == E_INVALID and "regulator" in msg
    finally:
        m._close()


@pytest.mark.parametrize("label,B,par", [
    ("a probability of 1.5", 2, ([0.1, 1.5], [0.5, 0.5], [0.0, 0.0], [1.0, 1.0])),
    ("a NaN", 2, ([0.1, 0.2], [0.5, 0.5], [0.0, np.nan], [1.0, 1.0])),
    ("a negative probability", 1, ([0.1], [0.5], [0.0], [-1e-9])),
    ("a NULL array", 2, ([0.1, 0.2], None, [0.0, 0.0], [1.0, 1.0])),
    ("a negative batch", -1, ([0.1], [0.5], [0.0], [1.0])),
])
def test_setter_rejects_bad_arguments_and_keeps_the_setting(host_handle, label, B, par):
    assert _set(host_handle, 1, [0.25], [0.5], [0.125], [1.0])[0] == 0
    try:
        rc, msg = _set(host_handle, B, *par)
        assert rc == E_INVALID and msg.startswith("tmpc_mc_set_channel: "), (label, rc, msg)
        assert np.array_equal(_native.mc_get_channel(host_handle, 1)[0], [[0.25, 0.25, 0.34375], [0.5, 0.5, 0.5625]])
    finally:
        _native.mc_set_channel(host_handle, None)


def test_run_and_open_need_the_channels_batch(host_handle):
    L = _native.lib()
    B, T = 4, 6
    z = np.zeros((B, T, host_handle.nx))
    ptr = z.ctypes.data
    out = [None] * 6

    def run(nb):
        return L.tmpc_mc_run(host_handle.ptr, nb, T, 0, None, ptr, ptr, ptr, ptr, None, None, None, 0, *out)

    def open_(nb):
        return L.tmpc_mc_open(host_handle.ptr, nb, T, 0, None, ptr, ptr, ptr, None, None, None, 0, None, None, 0, None, None, 0)
    assert run(B) == E_INVALID and "NULL argument" in host_handle.error()       # no channel: p_loss is needed
    _native.mc_set_channel(host_handle, montecarlo.burst_channel(0.3, 3.0), B=B)
    try:
        assert run(B - 1) == E_INVALID and "loss channel was set for B = 4" in host_handle.error()
        assert open_(B + 1) == E_INVALID and "loss channel was set for B = 4" in host_handle.error()
        assert run(B) == -3 and "host-only" in host_handle.error()              # p_loss NULL is fine now: only the device is missing
        assert open_(B) == -3
    finally:
        _native.mc_set_channel(host_handle, None)
    lost = np.zeros(B, np.int32)
    assert L.tmpc_mc_get_link_stats(host_handle.ptr, B, lost.ctypes.data, None, None, None) == E_INVALID      # nothing has run
    assert "tmpc_mc_get_link_stats" in host_handle.error()
    assert L.tmpc_mc_get_link_stats(None, B, None, None, None, None) == E_INVALID


def test_bindings_find_the_batch_and_leave_no_channel_behind(host_handle):
    """_native.mc_run / mc_open: a channel of scalars with nothing else that gives the batch is refused with a message (not run as
    one trajectory), and a call that is refused -- by the binding's shape checks or by the library -- leaves no channel on the handle."""
    h, L = host_handle, _native.lib()
    ch = dict(p_gb=0.1, p_bg=0.2, e_g=0.0, e_b=1.0)
    thr = np.zeros(18)

    def channel_set(B=3):
        return L.tmpc_mc_get_channel(h.ptr, B, thr.ctypes.data) == 0
    with pytest.raises(ValueError, match="does not say how many trajectories"):
        _native.mc_run(h, None, np.zeros(5), None, None, None, device_rng=(1, 0, np.zeros(h.nx)), channel=ch)
    with pytest.raises(ValueError, match="does not say how many trajectories"):
        _native.mc_open(h, None, np.zeros(5), device_rng=(1, 0), channel=ch)
    with pytest.raises(ValueError, match="p_loss or channel"):
        _native.mc_run(h, None, np.zeros(5), np.zeros((3, 5)), np.zeros((3, 5)), np.zeros((3, 5, h.nx)))
    # the batch from x0, from ref_id, from th_u, from a per-trajectory parameter
    assert _native.loop_batch("t", None, ch, x0=np.zeros((3, h.nx)), nx=h.nx)[2] == 3
    assert _native.loop_batch("t", None, ch, ref_id=np.zeros(6, np.int32))[2] == 6
    assert _native.loop_batch("t", None, ch, th_u=np.zeros((4, 9)))[2] == 4
    assert _native.loop_batch("t", None, dict(ch, e_g=[0.0, 0.1]))[2] == 2
    with pytest.raises(ValueError, match="inconsistent shapes"):
        _native.mc_run(h, None, np.zeros(5), np.zeros((3, 5)), np.zeros((3, 4)), np.zeros((3, 5, h.nx)), channel=ch)
    assert not channel_set()
    with pytest.raises(ValueError, match=r"one entry per trajectory \(3\)"):
        _native.mc_run(h, None, np.zeros(5), np.zeros((3, 5)), np.zeros((3, 5)), np.zeros((3, 5, h.nx)), channel=dict(ch, e_g=[0.0, 0.1]))
    assert not channel_set(2)
    with pytest.raises(RuntimeError, match="host-only"):          # the library's refusal: the channel had been set, and is cleared
        _native.mc_run(h, None, np.zeros(5), np.zeros((3, 5)), np.zeros((3, 5)), np.zeros((3, 5, h.nx)), channel=ch)
    assert not channel_set()
    with pytest.raises(RuntimeError, match="host-only"):
        _native.mc_open(h, None, np.zeros(5), np.zeros((3, 5)), np.zeros((3, 5)), channel=ch)
    assert not channel_set()


def test_sweep_refuses_bursts_at_loss_rate_one():
    with pytest.raises(ValueError, match="every loss rate below 1"):
        montecarlo.mc_sweep(None, dict(w_bound=np.zeros(2)), [0.0, 1.0], 2, 5, 0.5, mean_burst=3.0)


def test_python_channel_argument_forms():
    a = montecarlo.channel_parameters(dict(p_gb=0.1, p_bg=[0.5, 0.25, 1.0], e_g=0.0, e_b=1.0))
    assert all(v.shape == (3,) and v.dtype == np.float64 for v in a) and np.array_equal(a[1], [0.5, 0.25, 1.0])
    with pytest.raises(ValueError):
        montecarlo.channel_parameters(([0.1, 0.2], 0.2, 0.0, 1.0), 3)
    with pytest.raises(ValueError):
        montecarlo.channel_parameters((0.1, 1.2, 0.0, 1.0))
    with pytest.raises(ValueError):
        montecarlo.burst_channel(0.9, 2.0)                                      # p_gb would be 4.5
    ch = montecarlo.burst_channel([0.1, 0.5], [1.0, 12.0])
    assert np.allclose(ch["p_gb"] / (ch["p_gb"] + ch["p_bg"]), [0.1, 0.5]) and np.allclose(1.0 / ch["p_bg"], [1.0, 12.0])


# ------------------------------------------------------------------------------------------------ the host loops' link statistics
def _stub_loop(theta, gamma, N=3, channel=None, tracking=False, status=None):
    """The host loop around a stub controller (every packet: zeros) on the double integrator, the flags given as uniforms against
    p_loss = 1/2 (0: lost, 1: arrives)."""
    w = workloads.double_integrator()
    theta, gamma = np.atleast_2d(theta).astype(np.float64), np.atleast_2d(gamma).astype(np.float64)
    nb, T = theta.shape
    K = np.array([[0.5, 1.0]])
    Z = Polytope(np.r_[np.eye(2), -np.eye(2)], 1e6 * np.ones(4))

    def packets(x_hat, r, g=None):
        st = np.zeros(nb, dtype=np.int32) if status is None else status(len(calls))
        calls.append(1)
        return np.zeros((nb, 1, N + 1)), np.array(x_hat), st
    calls = []
    args = (np.full(nb, 0.5), np.zeros(T), theta, gamma, np.zeros((nb, T, 2)))
    if tracking:
        return montecarlo.run_remote_tracking_mpc(packets, w["A"], w["B"], K, N, *args, channel=channel)
    return montecarlo.run_remote_tube_mpc(packets, w["A"], w["B"], K, K, N, Z, *args, channel=channel)


def test_host_loop_link_statistics_on_a_hand_written_pattern():
    """N = 3.  Trajectory 0, every plant packet arrives: each arrival of the controller's packet is adopted (s_t = t), the gaps are
    0 1 2 0 1 2 3 4 5 0 1 0 -> max_gap 5, three steps at or past the end of the buffer (gap >= 3), eight packets lost.  Trajectory 1:
    both packets of step 2 are lost, so the controller of step 3 does not know of the loss (q = 1 < last loss 2): its packet arrives
    and is NOT adopted (SmartActuator.py:57-107) -> gaps 0 0 1 2 0 .. 0."""
    theta = np.array([[1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 1], [1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1]])
    gamma = np.array([[1] * 12, [1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1]])
    theta[0, 0] = 0                                                             # the draw of t = 0 is ignored: the packet arrives
    out = _stub_loop(theta, gamma)
    assert out["lost_up"].tolist() == [8, 1] and out["lost_down"].tolist() == [0, 1]
    assert out["max_gap"].tolist() == [5, 2] and out["overrun"].tolist() == [3, 0]
    assert all(out[k].dtype == np.int32 for k in ("lost_up", "lost_down", "max_gap", "overrun"))


def test_host_loop_all_lost_channel_and_failed_solves():
    T, N = 12, 3
    u = np.random.default_rng(0).uniform(size=(2, T))
    out = _stub_loop(u, u, N=N, channel=dict(p_gb=[1.0, 0.0], p_bg=0.0, e_g=0.0, e_b=1.0))
    assert out["max_gap"].tolist() == [T - 1, 0] and out["overrun"].tolist() == [T - N, 0]
    assert out["lost_up"].tolist() == [T - 1, 0] and out["lost_down"].tolist() == [T - 1, 0]
    # a failed solve (status 2) withholds the packet, but the CHANNEL dropped nothing: the gap grows, lost_up does not
    ones = np.ones((1, T))
    out = _stub_loop(ones, ones, N=N, status=lambda t: np.array([2 if t in (4, 5) else 0], dtype=np.int32))
    assert out["lost_up"].tolist() == [0] and out["max_gap"].tolist() == [2] and out["not_optimal"].tolist() == [2]
    # R-MPC: the trajectory stops at its infeasible solve (step 4) and counts nothing from there on
    zeros_after_0 = np.r_[1.0, np.zeros(T - 1)][None]
    out = _stub_loop(zeros_after_0, ones, N=N, tracking=True, status=lambda t: np.array([2 if t == 4 else 0], dtype=np.int32))
    assert out["infeasible"].tolist() == [True]
    assert out["lost_up"].tolist() == [3] and out["max_gap"].tolist() == [3] and out["overrun"].tolist() == [1]
