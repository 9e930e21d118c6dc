"""The regulator QPs of tmpc_create_regulator on host-only handles (device = -1): the C struct and its ctypes mirror, the
condensed form against the sparse QP written out in numpy (tests/regulator_problems.py), argument checking, and the resource
notes of the closed loop's step kernel.  CPU only."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import common
import regulator_problems as rp
from LinearMPCOverNetworks import _native

ROOT = os.path.dirname(common.PKG)
CTYPE = {"int32_t": C.c_int32, "double": C.c_double, "const double *": C.POINTER(C.c_double)}


def test_header_and_ctypes_mirror_agree():
    src = open(os.path.join(ROOT, "include", "tmpc.h")).read()
    body = re.search(r"typedef struct tmpc_regulator_problem \{(.*?)\} tmpc_regulator_problem;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    hdr = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        base, names = re.match(r"(const double|int32_t|double)\s+(.*)", decl).groups()
        for n in names.split(","):
            n = n.strip()
            hdr.append((n.lstrip("* "), CTYPE["const double *" if n.startswith("*") else base]))
    prod = list(_native.TmpcRegulatorProblem._fields_)
    assert [n for n, _ in hdr] == [n for n, _ in prod]
    for (n, th), (_, tp) in zip(hdr, prod):
        assert C.sizeof(th) == C.sizeof(tp) and issubclass(tp, C._Pointer) == issubclass(th, C._Pointer), n
    assert C.sizeof(_native.TmpcRegulatorProblem) == 9 * 4 + 4 + 8 + 14 * 8


def _host(kind):
    if kind == "plain_U":
        return rp.plain_double_integrator(X=False, U=True, device=-1)
    if kind == "plain_XU":
        return rp.plain_double_integrator(X=True, U=True, device=-1)
    if kind == "plain_free":
        return rp.plain_double_integrator(X=False, U=False, device=-1)
    return rp.mayne_tube(device=-1)


@pytest.mark.parametrize("kind", ["plain_U", "plain_XU", "plain_free", "mayne_tube"])
def test_condensed_form_equals_the_sparse_qp(kind, hip_lib):
    m = _host(kind)
    try:
        sp = rp.SparseQP(m)
        c = _native.get_condensed(m._handle)
        nv, nc, npar = _native.get_dims(m._handle)
        assert nv == sp.nv
        assert np.all(c["F2"] == 0.0)
        dep = sp.z_dependent_rows()
        assert nc == int(dep.sum()) and npar == int((~dep).sum())
        if kind == "plain_free":
            assert nc == 0 and npar == 0
        if kind == "plain_XU":
            assert npar > 0              # x_0 = x_k: its rows (and those x_k alone decides) are checked once, not iterated on
        rng = np.random.default_rng(7)
        scale = 3.0 if kind == "mayne_tube" else 2.0
        for _ in range(20):
            xk = scale * rng.standard_normal(sp.nx)
            z1, z2 = rng.standard_normal(sp.nv), rng.standard_normal(sp.nv)
            # objective: the condensed form drops the constant of x_k alone, so differences in z must agree
            qc = lambda z: 0.5 * z @ c["H"] @ z + (c["F1"] @ xk) @ z       # noqa: E731
            ds, dc = sp.cost(z1, xk) - sp.cost(z2, xk), qc(z1) - qc(z2)
            assert abs(ds - dc) <= 1e-12 * max(abs(sp.cost(z1, xk)), abs(sp.cost(z2, xk)), 1.0), (ds, dc)
            g_s, g_c = sp.cost_gradient(z1, xk), c["H"] @ z1 + c["F1"] @ xk
            assert np.max(np.abs(g_s - g_c)) <= 1e-12 * max(np.max(np.abs(g_s)), 1.0)
            # constraint slacks, the z-dependent rows in the reference's order
            s_c = c["G"] @ z1 - c["g0"] - c["E"] @ xk
            s_s = sp.rows(z1, xk)[dep]
            assert s_c.shape == s_s.shape
            if s_c.size:
                assert np.max(np.abs(s_c - s_s)) <= 1e-12 * max(np.max(np.abs(s_s)), 1.0)
    finally:
        m._close()


def test_cartpole_regulator_is_condensed(hip_lib):
    """The cart-pole model with its X and U regulated to the origin: a regulator of nx = 4; the kernel it lands on."""
    w = rp.workloads.cartpole()
    m = rp.RegulatorMPC(w["A"], w["B"], w["Q"], w["R"], 10)
    m.set_input_constraints(w["U"])
    m.set_state_constraints(w["X"])
    m.set_device(-1)
    m.generate_optimization_problem()
    try:
        nv, nc, npar = _native.get_dims(m._handle)
        assert nv == 10 and nc > 0
        assert _native.kernel_name(m._handle).startswith("tmpc::solve_kernel<")
    finally:
        m._close()


def _raw_problem(**over):
    A = np.array([[1.0, 1.0], [0.0, 1.0]])
    B = np.array([[0.5], [1.0]])
    Q, R, P, K = np.eye(2), 0.01 * np.eye(1), np.eye(2), np.array([[0.5, 1.0]])
    Hb, hb = np.r_[np.eye(2), -np.eye(2)], np.ones(4)
    d = dict(nx=2, nu=1, N=5, A=A, B=B, Q=Q, R=R, P=P, K=K, tube=1, HZ=Hb, hZ=hb, Hu=np.array([[1.0], [-1.0]]), hu=np.ones(2))
    d.update(over)
    return d


@pytest.mark.parametrize("over, words", [
    (dict(tube=1, HZ=None, hZ=None), "rZ > 0"),
    (dict(tube=0, HZ=None, hZ=None, Hf=np.eye(2), hf=np.ones(2)), "plain regulator"),
    (dict(K=None), "needs P and K"),
    (dict(nx=0), "0 < nx <= 16"),
    (dict(R=None), "must be given"),
])
def test_invalid_problems_are_reported(over, words, hip_lib):
    d = _raw_problem(**{k: v for k, v in over.items() if k != "nx"})
    p, keep = _native.pack_regulator_problem(d)
    if over.get("nx") == 0:
        p.nx = 0
    h = C.c_void_p()
    rc = _native.lib().tmpc_create_regulator(C.byref(p), -1, C.byref(h))
    assert rc == -1 and not h.value
    assert words in _native.lib().tmpc_last_error(None).decode()


def test_row_count_with_null_matrix_is_invalid(hip_lib):
    p, keep = _native.pack_regulator_problem(_raw_problem())
    p.rx = 3                                   # rows declared, Hx / hx NULL
    h = C.c_void_p()
    assert _native.lib().tmpc_create_regulator(C.byref(p), -1, C.byref(h)) == -1
    assert "NULL" in _native.lib().tmpc_last_error(None).decode()


def test_solve_arguments_of_a_regulator_handle(hip_lib):
    """ref may be NULL; xu_ss and variant must be NULL (checked before the device: a host-only handle answers E_DEVICE)."""
    m = rp.plain_double_integrator(device=-1)
    try:
        L, B, nx, N = _native.lib(), 2, 2, 10
        x = np.zeros((B, nx))
        u, x0, ss, st, it = np.empty((B, N)), np.empty((B, nx)), np.empty((B, nx + 1)), np.empty(B, np.int32), np.empty(B, np.int32)
        args = lambda ss_ptr: (m._handle.ptr, B, x.ctypes.data, None, None, u.ctypes.data, x0.ctypes.data, ss_ptr, None,  # noqa: E731
                               st.ctypes.data, it.ctypes.data)
        assert L.tmpc_solve_batch(*args(ss.ctypes.data)) == -1
        assert "xu_ss" in m._handle.error()
        assert L.tmpc_solve_batch(*args(None)) == -3          # E_DEVICE: the arguments were accepted
        assert L.tmpc_reg_run(m._handle.ptr, 1, 1, x.ctypes.data, None, None, None, 0, None, None, 0, None, None, 0,
                              *([None] * 8), -1, None, None, None) == -3
        assert L.tmpc_reg_run(m._handle.ptr, 1, 1, None, None, None, None, 0, None, None, 0, None, None, 0,
                              *([None] * 8), -1, None, None, None) == -1
    finally:
        m._close()


def test_tracking_handles_are_refused_by_the_regulator_loop(hip_lib):
    mpc, _ = common.make_mpc("double_integrator", 10, False)
    mpc._device = -1
    mpc.generate_optimization_problem(False)
    try:
        x = np.zeros(2)
        rc = _native.lib().tmpc_reg_run(mpc._handle.ptr, 1, 1, x.ctypes.data, None, None, None, 0, None, None, 0, None, None, 0,
                                        *([None] * 8), -1, None, None, None)
        assert rc == -1 and "regulator handle" in mpc._handle.error()
    finally:
        mpc._close()


def test_step_kernel_has_no_scratch():
    spec = importlib.util.spec_from_file_location("code_object_notes", os.path.join(ROOT, "scripts", "code_object_notes.py"))
    notes = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(notes)
    ks = notes.kernels(os.path.join(common.PKG, "lib", "libtmpc_hip.so"))
    dm = notes.demangle(list(ks))
    reg = {dm[n]: k for n, k in ks.items() if "reg_step_kernel" in dm[n]}
    assert len(reg) == 1, sorted(reg)
    (name, k), = reg.items()
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, k
    for word in ("mc_step_kernel", "mc_post_kernel", "mc_tube_kernel", "::solve_kernel<", "::closed_loop_kernel<",
                 "::closed_loop_step_kernel<", "::solve_block_kernel<"):
        assert word not in name
