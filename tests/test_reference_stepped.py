"""The stepped closed loop with full-state references (include/tmpc.h: tmpc_mc_set_reference_table before tmpc_mc_open;
tmpc_mc_step_device_ref / tmpc_mc_step_ref; ClosedLoopSession.step(x, ref_next)).  Where the same arithmetic runs twice the results
are compared as bytes; a session against tmpc_mc_run within the bands tests/test_stepped_loop.py uses for that pair."""
import numpy as np
import pytest

import common
from LinearMPCOverNetworks import _native, montecarlo
from test_reference_schedules import NB, P_LOSS, cartpole_table
from test_stepped_loop import _compare, _linear
from test_stepped_loop_api import E_INVALID, raw_open

pytestmark = pytest.mark.gpu

STATS = ("err2", "tube_violations", "x_violations", "u_violations", "not_optimal", "consistent", "iters_sum")
_MPC = {}


def _cartpole(extended=False):
    if extended not in _MPC:
        _MPC[extended] = common.make_mpc("cartpole", 10, True, extended=extended, create=True)
    return _MPC[extended]


def _case(w):
    tab, ids = cartpole_table()
    th, ga, dist = montecarlo.draw_realisations(NB, tab.shape[1], w["w_bound"], seed=11)
    return tab, ids, th, ga, dist


def _session(mpc, w, ref, th, ga, dist, ref_id=None, online=None, feed=None, device=False, **kw):
    """A session around the linear plant + dist[:, t].  online(t) -> the (B, nx) reference of the solve of step t + 1, or None;
    feed = (c, x_traj): trajectory c gets x_traj[t]; device: tensors through tmpc_mc_step_device_ref on torch's current stream."""
    nb, nt = th.shape
    plant = _linear(w)
    x = np.zeros((nb, mpc._nx))
    us = []
    if device:
        import torch
    with mpc.open_closed_loop(P_LOSS, ref, th, ga, T=nt, ref_id=ref_id, **kw) as s:
        for t in range(nt):
            if feed is not None:
                x[feed[0]] = feed[1][t]
            r = None if online is None else online(t)
            if device:
                xd = torch.as_tensor(x, device="cuda")
                u = s.step(xd, None if r is None else torch.as_tensor(np.ascontiguousarray(r), device="cuda")).cpu().numpy()
            else:
                u = s.step(x, r)
            us.append(u.copy())
            x = plant(x, u) + dist[:, t]
    out = dict(s.stats)
    out.update(x_final=x, u_all=np.array(us))
    return out


def _same(a, b, keys=STATS + ("x_final", "u_all")):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


# (a) a session in table mode against tmpc_mc_run with the table
@pytest.mark.parametrize("extended", [False, True])
def test_table_session_equals_the_run(hip_lib, extended):
    mpc, w = _cartpole(extended)
    tab, ids, th, ga, dist = _case(w)
    run = mpc.run_closed_loop(P_LOSS, tab, th, ga, dist, extended=extended, ref_id=ids, capture=7)
    ses = _session(mpc, w, tab, th, ga, dist, ref_id=ids, extended=extended)
    assert ses["steps"] == tab.shape[1] and np.all(ses["not_optimal"] == 0)
    _compare(f"cart-pole, 4 schedules, extended = {extended}", ses, run)
    # trajectory 7 of the run, recorded, fed to trajectory 7 of a session: the same inputs and statistics, byte for byte
    fed = _session(mpc, w, tab, th, ga, dist, ref_id=ids, extended=extended, feed=(7, run["x_traj"]))
    assert fed["u_all"][:, 7].tobytes() == run["u_traj"].tobytes()
    for k in ("err2", "tube_violations", "not_optimal", "iters_sum"):
        assert fed[k][7:8].tobytes() == run[k][7:8].tobytes(), k


# (b) row t + 1 handed over as ref_next = the NULL steps
@pytest.mark.parametrize("device", [False, True])
def test_next_row_as_ref_next_equals_the_plain_steps(hip_lib, device):
    mpc, w = _cartpole()
    tab, ids, th, ga, dist = _case(w)
    T = tab.shape[1]
    plain = _session(mpc, w, tab, th, ga, dist, ref_id=ids, device=device)
    given = _session(mpc, w, tab, th, ga, dist, ref_id=ids, device=device, online=lambda t: tab[ids, min(t + 1, T - 1)])
    _same(given, plain)


# (c) a constant table steered online through a schedule = a session opened on the schedule
def test_online_references_equal_the_schedule(hip_lib):
    mpc, w = _cartpole()
    tab, ids, th, ga, dist = _case(w)
    T = tab.shape[1]
    full = tab[ids]
    on_schedule = _session(mpc, w, full, th, ga, dist)
    const = np.broadcast_to(full[:, :1], full.shape)                  # row 0 for ever: the reference of step 0, then the caller's
    steered = _session(mpc, w, const, th, ga, dist, online=lambda t: full[:, min(t + 1, T - 1)])
    _same(steered, on_schedule)
    unsteered = _session(mpc, w, const, th, ga, dist)
    assert np.max(np.abs(unsteered["err2"] - on_schedule["err2"])) > 1e-6          # the online references matter


# (d) ref_next produced by torch on the caller's stream right before the step, nothing synchronised in between
def _torch_session(mpc, w, ref_open, sched, th, ga, dist, stream):
    """A session around the linear plant in torch (x, u, the plant and, with `sched` (T, B, nx), ref_next all on `stream`)."""
    import torch
    dev = torch.device("cuda", 0)
    T = th.shape[1]
    A, B = (torch.as_tensor(np.asarray(w[k], dtype=np.float64), device=dev) for k in ("A", "B"))
    wd = torch.as_tensor(np.ascontiguousarray(dist.transpose(1, 0, 2)), device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    us = []
    with torch.cuda.stream(stream):
        x = torch.zeros((NB, 4), dtype=torch.float64, device=dev)
        with mpc.open_closed_loop(P_LOSS, ref_open, th, ga, T=T) as s:
            for t in range(T):
                r = None
                if sched is not None:
                    half = sched[min(t + 1, T - 1)] * 0.5
                    r = (half + half).contiguous()                    # kernels on `stream`, in flight when the step is enqueued
                u = s.step(x, r)
                us.append(u.clone())
                x = (x @ A.T + u @ B.T + wd[t]).contiguous()
        out = dict(s.stats)
        out.update(x_final=x.cpu().numpy(), u_all=torch.stack(us).cpu().numpy())
    return out


def test_ref_next_computed_on_the_callers_stream(hip_lib):
    """(c) with everything on the device: the session opened on the schedule (torch's default stream) against the session opened on
    a constant table whose ref_next comes out of torch kernels on a side stream -- the same plant arithmetic on both sides, bytes;
    and the numpy-plant session of (c) within the bands of a session against a run (another matrix product rounds the plant)."""
    import torch
    mpc, w = _cartpole()
    tab, ids, th, ga, dist = _case(w)
    full = tab[ids]
    const = np.broadcast_to(full[:, :1], full.shape)
    dev = torch.device("cuda", 0)
    sched = torch.as_tensor(np.ascontiguousarray(full.transpose(1, 0, 2)), device=dev)            # (T, B, nx)
    want = _torch_session(mpc, w, full, None, th, ga, dist, torch.cuda.current_stream(dev))
    got = _torch_session(mpc, w, const, sched, th, ga, dist, torch.cuda.Stream(device=dev))
    _same(got, want)
    _compare("torch plant and online references against the numpy plant on the schedule", got, _session(mpc, w, full, th, ga, dist))


# (e), (f): the refusals
def test_ref_next_needs_a_table_session_and_leaves_the_session_usable(hip_lib):
    mpc, w = _cartpole()
    _, _, th, ga, dist = _case(w)
    T = th.shape[1]
    ref = np.where(np.arange(T) < T // 2, 0.5, -0.3)
    want = _session(mpc, w, ref, th, ga, dist)
    h, L = mpc._handle, _native.lib()
    x, u, r = np.zeros((NB, 4)), np.zeros((NB, 1)), np.zeros((NB, 4))
    plant = _linear(w)
    us = []
    with mpc.open_closed_loop(P_LOSS, ref, th, ga) as s:
        for t in range(T):
            if t in (0, 5):
                assert L.tmpc_mc_step_ref(h.ptr, x.ctypes.data, u.ctypes.data, r.ctypes.data) == E_INVALID
                assert "tmpc_mc_step_ref" in h.error() and "reference table" in h.error()
                assert L.tmpc_mc_step_device_ref(h.ptr, x.ctypes.data, u.ctypes.data, r.ctypes.data, None) == E_INVALID
                assert "tmpc_mc_step_device_ref" in h.error()
                with pytest.raises(RuntimeError, match="reference table"):
                    s.step(x, r)
            ut = s.step(x)
            us.append(ut.copy())
            x = plant(x, ut) + dist[:, t]
    out = dict(s.stats)
    out.update(x_final=x, u_all=np.array(us))
    _same(out, want)


def test_table_bounds_the_loops_and_the_setter_waits_for_the_session(hip_lib):
    mpc, w = _cartpole()
    tab, ids, th, ga, dist = _case(w)
    h, T = mpc._handle, tab.shape[1]
    try:
        _native.mc_set_reference(h, tab, ids)
        rc, msg = raw_open(h, NB + 1, T)
        assert rc == E_INVALID and msg.startswith("tmpc_mc_open: ") and str(NB + 1) in msg and str(NB) in msg
        rc, msg = raw_open(h, NB, T + 1)
        assert rc == E_INVALID and msg.startswith("tmpc_mc_open: ") and str(T + 1) in msg and str(T) in msg
        keep = [np.zeros(NB + 1), np.zeros((NB + 1, T + 1)), np.zeros((NB + 1, T + 1)), np.zeros((NB + 1, T + 1, 4))]
        pl, thz, gaz, wz = [a.ctypes.data for a in keep]
        for B_, T_, number in ((NB - 1, T, NB - 1), (NB, T + 1, T + 1)):
            rc = _native.lib().tmpc_mc_run(h.ptr, B_, T_, 0, pl, None, thz, gaz, wz, None, None, None, 0, *([None] * 6))
            assert rc == E_INVALID and h.error().startswith("tmpc_mc_run: ") and str(number) in h.error(), h.error()
        rc, msg = raw_open(h, NB, T, ref=None, p_loss=P_LOSS)                     # `ref` is not read with a table
        assert rc == 0, msg
        assert _native.lib().tmpc_mc_set_reference_table(h.ptr, 0, 0, None, 0, None) == E_INVALID
        assert "tmpc_mc_set_reference_table" in h.error() and "tmpc_mc_close" in h.error()
        assert _native.lib().tmpc_mc_close(h.ptr, *([None] * 8)) == 0
    finally:
        _native.mc_set_reference(h, None)
    out = mpc.run_closed_loop(P_LOSS, tab[0, :, 0], th, ga, dist)               # the handle is as before
    assert np.all(out["not_optimal"] == 0)
