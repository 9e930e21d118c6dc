"""Lane packing of the wave kernel's layout (csrc/tmpc_api.cpp: upload_wave): the functionals of a partly filled last
factored slot sit on idle lanes of the dense paired slots, and the kernel skips the emptied slot (DeviceQP::ncs).  CPU part: the kernel's
source on the host execution model (tests/wavesim) under MemorySanitizer, on the packed layout and on the layout
TMPC_NO_LANE_PACKING=1 keeps.  A row side of the skipped slot that is read before it is written is what MemorySanitizer is there to
catch; an answer that depends on one differs from the oracle's."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import common
from LinearMPCOverNetworks import _native
from oracle.oracle import Oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "wavesim"))

ATOL_U = 1e-8          # tests/test_hip_parity.py
S = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))
CONTINUATION_STATE = 587          # tests/test_residual_scale_gpu.py: the fixture state whose first hand-over is not certified


def _cases():
    """24 fixture states (the continuation state among them), the infeasible and the trivially optimal edge case of
    tests/test_residual_scale_gpu.py"""
    idx = np.r_[np.arange(0, 600, 26), CONTINUATION_STATE]
    assert len(idx) == 25 and len(set(idx)) == 25
    X = np.r_[S[idx, :4], [[0.0, 0.0, 0.2, 0.0], [0.5, 0.0, 0.0, 0.0]]]
    R = np.r_[S[idx, 4:], [[0.5, 0, 0, 0.0], [0.5, 0, 0, 0.0]]]
    return X, R


def test_layout_the_handle_reports(hip_lib, monkeypatch):
    """Host-only handles: the bench problem packs (46 dense and 206 factored pairs: the 14 of the fourth factored slot go to the 18 idle dense lanes), N = 11 is one lane short, the
    packet-received problem cannot empty a slot."""
    def factoring(N, extended=False):
        mpc, _ = common.make_mpc("cartpole", N, True, extended=extended, create=False)
        h = _native.create(mpc._problem_dict(), -1)
        try:
            return [_native.get_factoring(h, k) for k in range(2 if extended else 1)], [_native.get_dims(h, k)[1] for k in range(2 if extended else 1)]
        finally:
            _native.destroy(h)
    assert factoring(10) == ([(120, 384, 5)], [504])
    assert factoring(11) == ([(102, 412, 5)], [514])
    assert factoring(10, extended=True) == ([(120, 384, 5), (102, 854, 4)], [504, 956])
    monkeypatch.setenv("TMPC_NO_LANE_PACKING", "1")
    assert factoring(10) == ([(92, 412, 5)], [504])
    assert factoring(10, extended=True) == ([(92, 412, 5), (102, 854, 4)], [504, 956])


def test_packed_and_unpacked_layouts_on_the_host_model_under_memory_sanitizer(oracle_lib, monkeypatch, tmp_path_factory):
    """The stand-alone MemorySanitizer build of the kernel source (tests/wavesim/Makefile: wavesim_msan; registers, LDS and outputs start
    out poisoned), both layouts, the cases in four processes each."""
    import hostsim
    import run_case
    binary = hostsim.binaries_or_skip(tmp_path_factory, "wavesim", ["msan"], extra=run_case.EXTRA)["wavesim_msan"]
    mpc, _ = common.make_mpc("cartpole", 10, True, create=False)
    d = mpc._problem_dict()
    X, R = _cases()
    ref = Oracle(d).solve(X, R)
    assert list(ref["status"][-2:]) == [2, 0] and np.all(ref["status"][:-2] == 0) and ref["iters"][-1] == 0
    ok = ref["status"] == 0
    parts = np.array_split(np.arange(len(X)), 4)
    for packed in (True, False):
        if not packed:
            monkeypatch.setenv("TMPC_NO_LANE_PACKING", "1")
        h = _native.create(d, -1)
        try:
            assert _native.get_factoring(h, 0) == ((120, 384, 5) if packed else (92, 412, 5))
        finally:
            _native.destroy(h)
        # (run_case.run lays its own host-only handle out under the same environment)
        with ThreadPoolExecutor(len(parts)) as ex:
            outs = list(ex.map(lambda ii: run_case.run(binary, d, X[ii], R[ii], env=hostsim.SAN_ENV), parts))
        for ii, o in zip(parts, outs):
            hostsim.assert_clean(o["stderr"])
            assert np.array_equal(o["status"], ref["status"][ii]), (packed, o["status"], ref["status"][ii])
            good = ok[ii]
            err = np.max(np.abs(o["u_nom"][good] - ref["u_nom"][ii][good]))
            print(f"{'packed' if packed else 'unpacked'}: max |u_nom - oracle| {err:.2e}")
            assert err <= ATOL_U, (packed, err)
            assert np.all(np.isnan(o["u_nom"][~good]))
