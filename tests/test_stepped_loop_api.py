"""The stepped closed loop (include/tmpc.h: tmpc_mc_open / tmpc_mc_step_device / tmpc_mc_step / tmpc_mc_close) without a GPU: the
exports and their bindings, and every answer the entry points give before they touch a device."""
import ctypes as C

import numpy as np
import pytest

import common
from LinearMPCOverNetworks import _native

E_INVALID, E_DEVICE = -1, -3          # include/tmpc.h


def raw_open(h, B, T, extended=0, p_loss=True, ref=True, th=True, ga=True, x0=None, Z=None, X=None, U=None, rZ=None, rX=None, rU=None):
    """tmpc_mc_open with plain arrays -> (return code, message).  True: an array of the right size; None: NULL; rX etc.: a row
    count that overrides the arrays'."""
    keep = []

    def arr(v, shape):
        if v is None:
            return None
        a = np.zeros(shape) if v is True else np.ascontiguousarray(v, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data
    nb, nt = max(B, 1), max(T, 1)
    args = [arr(p_loss, nb), arr(ref, nt), arr(th, (nb, nt)), arr(ga, (nb, nt)), arr(x0, (nb, h.nx))]
    for P, r, dim in ((Z, rZ, h.nx), (X, rX, h.nx), (U, rU, h.nu)):
        if P is None:
            args += [None, None, 0 if r is None else r]
        else:
            HA, hb = arr(P[0], None), arr(P[1], None)
            args += [HA, hb, np.asarray(P[0]).shape[0] if r is None else r]
    rc = _native.lib().tmpc_mc_open(h.ptr, B, T, extended, *args)
    return rc, h.error()


@pytest.fixture(scope="module")
def host_handles(hip_lib):
    """Host-only handles (device < 0) of the cart-pole at N = 10: the plain controller (one problem) and the extended one."""
    plain, _ = common.make_mpc("cartpole", 10, True, create=True, device=-1)
    ext, _ = common.make_mpc("cartpole", 10, True, extended=True, create=True, device=-1)
    yield plain._handle, ext._handle
    plain._close()
    ext._close()


def test_exports_exist_and_are_bound(hip_lib):
    L = _native.lib()
    for name, nargs in (("tmpc_mc_open", 18), ("tmpc_mc_step_device", 4), ("tmpc_mc_step", 3), ("tmpc_mc_close", 9)):
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == nargs, name
    for name in ("mc_open", "mc_step", "mc_close"):
        assert callable(getattr(_native, name))
    from LinearMPCOverNetworks.TubeTrackingMPC import ClosedLoopSession, TubeTrackingMPC
    assert callable(TubeTrackingMPC.open_closed_loop) and hasattr(ClosedLoopSession, "step") and hasattr(ClosedLoopSession, "close")
    src = open(common.ROOT + "/include/tmpc.h").read()
    assert "#define TMPC_PLANT_EXTERNAL 2" in src


def test_open_on_a_host_only_handle_needs_the_device(host_handles):
    plain, ext = host_handles
    rc, msg = raw_open(plain, 4, 10)
    assert rc == E_DEVICE and "host-only" in msg
    rc, msg = raw_open(ext, 4, 10, extended=1)
    assert rc == E_DEVICE and "host-only" in msg


@pytest.mark.parametrize("label,kw", [
    ("no loss rates", dict(p_loss=None)),
    ("no reference", dict(ref=None)),
    ("no theta uniforms", dict(th=None)),
    ("no gamma uniforms", dict(ga=None)),
    ("negative batch", dict(B=-1)),
    ("negative steps", dict(T=-3)),
    ("negative rows", dict(rX=-1)),
    ("rX without arrays", dict(rX=2)),
    ("rU without arrays", dict(rU=1)),
    ("rZ without arrays", dict(rZ=4)),
    ("extended on one problem", dict(extended=1)),
])
def test_open_rejects_bad_arguments_with_a_message(host_handles, label, kw):
    plain, _ = host_handles
    kw = dict(kw)
    B, T = kw.pop("B", 4), kw.pop("T", 10)
    rc, msg = raw_open(plain, B, T, **kw)
    assert rc == E_INVALID and msg.startswith("tmpc_mc_open: "), (label, rc, msg)


def test_open_on_a_null_handle_is_invalid(hip_lib):
    assert _native.lib().tmpc_mc_open(None, 1, 1, 0, *([None] * 7), 0, None, None, 0, None, None, 0) == E_INVALID


def test_step_and_close_without_a_session_are_invalid(host_handles):
    plain, _ = host_handles
    L = _native.lib()
    x, u = np.zeros((4, plain.nx)), np.zeros((4, plain.nu))
    assert L.tmpc_mc_step(plain.ptr, x.ctypes.data, u.ctypes.data) == E_INVALID and "no stepped closed loop is open" in plain.error()
    assert L.tmpc_mc_step_device(plain.ptr, x.ctypes.data, u.ctypes.data, None) == E_INVALID and "tmpc_mc_step_device" in plain.error()
    assert L.tmpc_mc_close(plain.ptr, *([None] * 8)) == E_INVALID and "tmpc_mc_close" in plain.error()
    for f, n in ((L.tmpc_mc_step, 2), (L.tmpc_mc_step_device, 3), (L.tmpc_mc_close, 8)):
        assert f(None, *([None] * n)) == E_INVALID


def test_native_step_checks_the_array_against_the_session(host_handles):
    """tmpc_mc_step copies B * nx entries out of x: the binding refuses an array of another size before the library sees it."""
    plain, _ = host_handles
    info = dict(B=4, T=10)
    for x in (np.zeros((3, plain.nx)), np.zeros(4 * plain.nx + 1)):
        with pytest.raises(ValueError, match="B \\* nx"):
            _native.mc_step(plain, info, x)
    with pytest.raises(ValueError, match="B \\* nu"):
        _native.mc_step(plain, info, np.zeros((4, plain.nx)), np.zeros(3 * plain.nu))
    with pytest.raises(RuntimeError, match="no stepped closed loop is open"):      # the right sizes reach the library
        _native.mc_step(plain, info, np.zeros((4, plain.nx)))


def test_set_plant_refuses_the_external_plant(host_handles):
    plain, _ = host_handles
    par = (C.c_double * 7)(1, 0.1, 0, 0.001, 9.8, 0.5, 0.02)
    assert _native.lib().tmpc_mc_set_plant(plain.ptr, 2, par, 10) == E_INVALID


def test_session_kernel_has_no_private_segment():
    """The state machines around the caller's plant: like mc_step_kernel, no private arrays, no spills."""
    from test_code_objects import _kernels
    ks = [k for n, k in _kernels().items() if "mc_session_kernel" in n]
    assert len(ks) == 1 and ks[0][".private_segment_fixed_size"] == 0 and ks[0][".vgpr_spill_count"] == 0
