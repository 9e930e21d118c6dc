"""The DEVICE state machines (mcstep::mc_step_wave through mc_step_kernel, what tmpc_mc_run launches behind every solve) with
several inputs and wide states, against the naive reference of tests/glue_reference.py.

tmpc_mc_replay feeds given packets, arrival flags and disturbances to the kernel; no QP is solved, so a deviation is the
state machines' (device, or -- tests/test_glue_reference.py on the same cases -- twin or reference).  With nu = 1, which is
all the recordings of the reference have, row-major and column-major B, K, K_anc coincide, the packet strides
(N + 1) nu and 3 nx + nu hide a swapped index, and the packet copy never takes its second pass (N nu > 64).

Shapes (glue_reference.SHAPES), each with the consistent actuator + estimator, the extended pair and the plain smart
actuator; 12 trajectories of 40 steps, loss rates 0 / 0.3 / 0.9, x0 non-zero, ancillary gain 0.8 K:
    (3, 2, 4)     smallest several-input case
    (2, 3, 5)     nu > nx; at N = 4 (glue_reference.horizon: tmpc_create refuses N = 5)
    (7, 2, 6)     nx past one Philox block boundary
    (12, 4, 30)   BASELINE config 5, N nu = 120; the extended pair at N = 28 (glue_reference.horizon: nv <= 128), N nu = 112
    (16, 16, 5)   both limits
Integers exactly, floats to 1e-12 of the trajectory's scale (the band of tests/test_device_glue_replay.py: the same sums in
another order)."""
import numpy as np
import pytest

import common  # noqa: F401  (sys.path)
import glue_reference as gr
from LinearMPCOverNetworks import _native
from LinearMPCOverNetworks.RegulatorMPC import RegulatorMPC

CASES = [(nx, nu, gr.horizon(nx, nu, N, kind), kind) for nx, nu, N in gr.SHAPES for kind in gr.KINDS]


@pytest.mark.gpu
@pytest.mark.parametrize("nx,nu,N,kind", CASES, ids=[f"nx{a}_nu{b}_N{c}_{k}" for a, b, c, k in CASES])
def test_device_state_machines_equal_the_naive_reference(hip_lib, nx, nu, N, kind):
    model, case, want = gr.reference(nx, nu, N, kind)
    ext = kind == "extended"
    h = _native.create(gr.box_problem(model, ext), device=0)
    try:
        assert (h.nx, h.nu, h.N) == (nx, nu, model["N"])
        got = _native.mc_replay(h, case["U"], case["theta"], case["gamma"], case["w"], xn0=case["xn0"] if ext else None,
                                x0=case["x0"], extended=ext, smart=kind == "smart")
    finally:
        _native.destroy(h)
    gr.compare(got, want, f"device nx={nx} nu={nu} N={model['N']} {kind}")
    gr.check_inputs(model, case, want)
    if (nx, nu) == (12, 4):
        assert model["N"] * nu > 64                      # the packet copy takes its second pass


def _refused(call, h, who):
    _native.kernel_ms_total(h, reset=True)
    _native.lane_counters(h, reset=True)
    with pytest.raises(RuntimeError, match=who + r" failed \(-2\).*nu <= 16"):        # TMPC_E_UNSUPPORTED
        call()
    assert _native.kernel_ms_total(h)[1] == 0 and _native.lane_counters(h)[0] == (0, 0)


@pytest.mark.gpu
def test_seventeen_inputs_are_refused_before_any_launch(hip_lib):
    """nu <= 16 in the state-machine kernels (one lane per input, LDS rows of 16), while tmpc_create takes any nu: on a tracking
    handle (nx = 16, nu = 17) and a regulator handle (nx = 2, nu = 17) tmpc_mc_run, tmpc_mc_replay and tmpc_reg_run answer
    TMPC_E_UNSUPPORTED with nothing enqueued."""
    model = gr.random_model(16, 17, 1, seed=1)
    h = _native.create(gr.box_problem(model, False), device=0)
    try:
        nb, T = 4, 3
        z = np.zeros((nb, T))
        _refused(lambda: _native.mc_run(h, np.zeros(nb), np.zeros(T), z, z, np.zeros((nb, T, 16))), h, "tmpc_mc_run")
        _refused(lambda: _native.mc_replay(h, np.zeros((nb, T, 2, 17)), z + 1, z + 1, np.zeros((nb, T, 16))), h, "tmpc_mc_replay")
    finally:
        _native.destroy(h)
    nx, nu = 2, 17
    m = RegulatorMPC(np.array([[1.0, 1.0], [0.0, 1.0]]), np.random.default_rng(3).standard_normal((nx, nu)), np.eye(nx), np.eye(nu), 2)
    m.generate_optimization_problem()
    try:
        _refused(lambda: m.run_closed_loop(np.ones((4, nx)), 3, w=np.zeros((4, 3, nx))), m._handle, "tmpc_reg_run")
        assert np.all(m._solve_regulator(np.ones((4, nx)))["status"] == 0)       # the handle itself is sound
    finally:
        m._close()
