"""The closed loops of one handle share their set-up (csrc/tmpc_loops.cpp: one arena, one list of its pieces, one record of the last
loop): nothing of a loop may reach the next one.  Three loops with different options run one after the other on ONE handle and, each
alone, on three fresh handles; the same arithmetic runs twice, so every returned array is compared as bytes."""
import numpy as np
import pytest

import common
from LinearMPCOverNetworks import montecarlo

pytestmark = pytest.mark.gpu

NB, T = 3, 4
P_LOSS = np.array([0.0, 0.3, 0.9])
REF = np.array([0.5, 0.5, -0.3, -0.3])


def _three_loops(mpcs, w, extended):
    """Loop k on mpcs[k] -> the three results.  1: tmpc_mc_run with the device generator, a loss channel and a reference schedule per
    trajectory; 2: a session (open, T steps around the linear plant, close) with host draws, independent losses and the (T,) reference;
    3: tmpc_mc_run with host draws, warm start and a recorded trajectory, independent losses."""
    A, Bm = np.asarray(w["A"], dtype=np.float64), np.asarray(w["B"], dtype=np.float64)
    nx = A.shape[0]
    th, ga, dist = montecarlo.draw_realisations(NB, T, w["w_bound"], seed=5)
    table = np.zeros((NB, T, nx))
    table[:, :, 0] = np.linspace(-0.4, 0.4, NB)[:, None] * np.linspace(1.0, 0.5, T)[None, :]
    first = mpcs[0].run_closed_loop(None, table, device_rng=(11, 2, w["w_bound"]), channel=montecarlo.burst_channel([0.2, 0.4, 0.6], 2.0),
                                    extended=extended)
    x, us = np.zeros((NB, nx)), []
    with mpcs[1].open_closed_loop(P_LOSS, REF, th, ga, extended=extended) as s:
        for t in range(T):
            u = s.step(x)
            us.append(u.copy())
            x = x @ A.T + u @ Bm.T + dist[:, t]
    second = dict(s.stats, u_all=np.array(us))
    third = mpcs[2].run_closed_loop(P_LOSS, REF, th, ga, dist, extended=extended, warm_start=True, capture=1)
    return first, second, third


def _same_bytes(label, got, want):
    assert sorted(got) == sorted(want), (label, sorted(got), sorted(want))
    for k, v in want.items():
        if isinstance(v, dict):
            _same_bytes(f"{label}.{k}", got[k], v)
        elif isinstance(v, np.ndarray):
            assert got[k].dtype == v.dtype and got[k].shape == v.shape and got[k].tobytes() == v.tobytes(), (label, k, got[k], v)
        else:
            assert got[k] == v, (label, k, got[k], v)


@pytest.mark.parametrize("extended", [False, True])
def test_loops_in_sequence_on_one_handle_equal_loops_on_fresh_handles(hip_lib, extended):
    made = [common.make_mpc("cartpole", 10, True, extended=extended, create=True) for _ in range(4)]
    mpcs, w = [m for m, _ in made], made[0][1]
    try:
        shared = _three_loops([mpcs[0]] * 3, w, extended)
        fresh = _three_loops(mpcs[1:], w, extended)
    finally:
        for m in mpcs:
            m._close()
    assert shared[1]["steps"] == T and shared[2]["x_traj"].shape == (T, mpcs[0]._nx)
    for k, name in enumerate(("run: device draws, channel, table", "session: host draws", "run: host draws, warm start, capture")):
        _same_bytes(name, shared[k], fresh[k])
