"""Every compiled QP kernel instantiation at its edges (the case table of tests/shape_cases.py), on the MI355X:

* an independent reference on a batch of 256 mixed states -- the KKT certificate of the un-condensed QP, the distance of u_0 to
  the exact minimiser on the certified active set, HiGHS on every infeasible answer (tests/certificates.py) -- and, for the
  tracking controllers, the CPU oracle;
* the wave kernel against the block kernel on every wave case;
* batch-size edges around the shape's wavefronts per workgroup, and a permuted batch;
* the closed-loop twins of every wave shape a tracking case reaches (fused == per step, bit for bit), and the regulator's
  device loop against a host loop of per-step solves.

Every case prints one line: case, kernel, optimal / infeasible instances, worst du_0, worst |u - oracle|."""
import numpy as np
import pytest

import certificates
import common
import regulator_problems as rp
import shape_cases
from LinearMPCOverNetworks import montecarlo
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

CASES = shape_cases.CASES
WAVE = [c for c in CASES if c.wave]
TRACK_WAVE = [c for c in WAVE if not c.regulator]
REG = [c for c in CASES if c.regulator]
_SOLVED = {}


def _ids(cases):
    return [c.id for c in cases]


@pytest.fixture(scope="module", autouse=True)
def _handles(hip_lib, oracle_lib):
    yield
    for m, *_ in _SOLVED.values():
        m._close()
    _SOLVED.clear()


def _solve(case, m, X, R, var):
    return m._solve_regulator(X) if case.regulator else m._solve(X, R, var)


def _solved(case):
    """(controller, X, R, variant, output of the full batch), built and solved once per case."""
    if case.id not in _SOLVED:
        m = case.build(device=0)
        X, R, var = case.states(m)
        _SOLVED[case.id] = (m, X, R, var, _solve(case, m, X, R, var))
    return _SOLVED[case.id]


def _statuses_agree(a, b):
    """The oracle's refinement is the weaker of the two: where it stops at "inaccurate" (1) the kernel may be optimal (0);
    an instance without a feasible point may end as "infeasible" in one and "numerical" in the other (test_random_models.py)."""
    return (a == b) | ((b == 1) & (a == 0)) | ((a >= 2) & (b >= 2))


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_against_the_references(case):
    m, X, R, var, out = _solved(case)
    st = out["status"]
    if case.regulator:
        c = certificates.certify_regulator(m, X, out)
        du0, dor = c["worst_du0"], float("nan")
    else:
        c = certificates.certify_outputs(m, X, R, out, var)
        du0 = c["worst"]["du0"]
        orc = Oracle(m._problem_dict())
        ref = orc.solve(X, R, var) if case.extended else orc.solve(X, R)
        rs = ref["status"]
        agree = _statuses_agree(st, rs)
        # the oracle may stop at "inaccurate" on an instance without any feasible point; the library's verdict must then be
        # proven outright by HiGHS
        for k in np.flatnonzero(~agree & (st == 2) & (rs == 1)):
            agree[k] = certificates.proven_infeasible(m, X[k], R[k], None if var is None else var[k])
        assert agree.all(), (case.id, np.flatnonzero(~agree), st[~agree], rs[~agree])
        ok = (st == 0) & (rs == 0)
        dor = float(np.max(np.abs(out["u_nom"][ok] - ref["u_nom"][ok]), initial=0.0))
        off = ok & ((np.abs(out["u_nom"] - ref["u_nom"]).reshape(len(X), -1).max(axis=1) > 1e-8) |
                    (np.abs(out["xu_ss"] - ref["xu_ss"]).max(axis=1) > 1e-9) |
                    (np.abs(out["x_nom"] - ref["x_nom"]).reshape(len(X), -1).max(axis=1) > 1e-8))
        # where the two differ by more than the parity bands, the library must sit on the exact minimiser and the oracle off it
        # (the oracle's refinement is the weaker of the two)
        for k in np.flatnonzero(off):
            v = None if var is None else var[k]
            dk = certificates.exact_distance(m, X[k], R[k], v, out["x_nom"][k], out["u_nom"][k], out["x_ss"][k], out["u_ss"][k])
            do = certificates.exact_distance(m, X[k], R[k], v, ref["x_nom"][k], ref["u_nom"][k], ref["x_ss"][k], ref["u_ss"][k])
            assert dk["certified"] and dk["u"] <= 1e-9 and dk["ss"] <= 1e-10 and dk["x"] <= 1e-9, (case.id, k, dk, do)
            assert do["u"] > 1e-8 or do["ss"] > 1e-9 or do["x"] > 1e-8, (case.id, k, dk, do)
        good = ok & ~off
        assert off.sum() <= 2, (case.id, np.flatnonzero(off))
        np.testing.assert_allclose(out["u_nom"][good], ref["u_nom"][good], atol=1e-8, rtol=0, err_msg=case.id)
        np.testing.assert_allclose(out["xu_ss"][good], ref["xu_ss"][good], atol=1e-9, rtol=0, err_msg=case.id)
        np.testing.assert_allclose(out["x_nom"][good], ref["x_nom"][good], atol=1e-8, rtol=0, err_msg=case.id)
        if off.any():
            print(f"\n{case.id}: instances {list(np.flatnonzero(off))}: the library on the exact minimiser, the oracle off it")
    print(f"\n{case.id}: {' + '.join(case.kernels)}: {c['n_opt']} optimal, {c['n_inf']} infeasible, "
          f"{int((out['iters'] == 0).sum())} without iteration, worst du0 {du0:.1e}, worst |u - oracle| {dor:.1e}")
    # the batch mixes what it is meant to: enough optimal instances to mean something, and (every case has states outside X)
    # infeasible ones
    assert c["n_opt"] >= 96 and c["n_inf"] >= 8, (case.id, c["n_opt"], c["n_inf"])


@pytest.mark.parametrize("case", WAVE, ids=_ids(WAVE))
def test_wave_equals_block(case):
    m, X, R, var, out = _solved(case)
    m.set_kernel_path("block")
    try:
        assert all(m.get_kernel_path(v) == "block" for v in range(len(case.kernels)))
        blk = _solve(case, m, X, R, var)
    finally:
        m.set_kernel_path(case.path)
    a, b = out["status"], blk["status"]
    # certified-optimal vs uncertified (status 1) may differ between the implementations; infeasibility may not
    agree = (a == b) | ((a <= 1) & (b <= 1))
    assert agree.all(), (case.id, np.flatnonzero(~agree), a[~agree], b[~agree])
    ok = (a == 0) & (b == 0)
    assert ok.sum() >= 96
    err = float(np.max(np.abs(blk["u_nom"][ok] - out["u_nom"][ok])))
    print(f"\n{case.id}: wave vs block: {int(ok.sum())} optimal in both, max |du| {err:.1e}")
    assert err <= 1e-9, (case.id, err)


def _per_block(case):
    """Wavefronts per workgroup of the case's kernel (the last template argument of solve_kernel; 1 for the block kernel)."""
    k = case.kernels[0]
    return int(k[k.rindex(",") + 1:-1]) if "::solve_kernel<" in k else 1


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_batch_size_edges(case):
    """A batch of 1, one wavefront short of a workgroup, one past it, and the permuted full batch: every instance gets the
    answer it gets in the full batch."""
    m, X, R, var, out = _solved(case)
    wpb = _per_block(case)
    rng = np.random.default_rng(17)
    perm = rng.permutation(len(X))
    # the hardest instances first: most iterations among the optimal ones, then an infeasible one
    hard = np.r_[np.argsort(-np.where(out["status"] == 0, out["iters"], -1), kind="stable")[:4],
                 np.flatnonzero(out["status"] == 2)[:1]]
    order = np.r_[hard, np.setdiff1d(perm, hard, assume_unique=True)]
    for idx in [order[:n] for n in sorted({1, max(wpb - 1, 1), wpb + 1})] + [perm]:
        sub = _solve(case, m, X[idx], None if R is None else R[idx], None if var is None else var[idx])
        # an instance's arithmetic does not depend on its neighbours or its position: the same bits
        assert np.array_equal(sub["status"], out["status"][idx]), (case.id, len(idx))
        assert np.array_equal(sub["u_nom"], out["u_nom"][idx], equal_nan=True), (case.id, len(idx))
        assert np.array_equal(sub["x_nom0"], out["x_nom0"][idx], equal_nan=True), (case.id, len(idx))


KEYS = ("err2", "tube_violations", "not_optimal", "x_final", "consistent", "iters_sum", "x_traj", "x_nom_traj", "u_traj")


@pytest.mark.parametrize("case", TRACK_WAVE, ids=_ids(TRACK_WAVE))
def test_closed_loop_twins(case):
    """closed_loop_kernel<shape> (one launch for the whole loop) and, for the extended controller, closed_loop_step_kernel<shape>
    of both problems (the state machines inside the solve launches) against a solve launch + state-machine launch per step:
    the same numbers, bit for bit (tests/test_fused_closed_loop.py on the shapes it does not reach)."""
    m, *_ = _solved(case)
    w = common.workload(case.name)
    nb, T = 40, 16
    p_loss = np.tile(np.arange(10) / 10.0, nb // 10)
    th, ga, dist = montecarlo.draw_realisations(nb, T, w["w_bound"], seed=41 + case.N)
    amp = 0.5 if case.name == "cartpole" else 4.0
    ref = np.where(np.arange(T) < T // 2, amp, -0.6 * amp)
    kw = dict(extended=True) if case.extended else {}
    off = m.run_closed_loop(p_loss, ref, th, ga, dist, capture=3, fused="off", **kw)
    on = m.run_closed_loop(p_loss, ref, th, ga, dist, capture=3, fused="on", **kw)
    if case.extended:
        assert off["loop_mode"] == 0 and on["loop_mode"] == 2
    else:
        assert on["fused"] and not off["fused"]
    for k in KEYS:
        assert np.array_equal(np.asarray(on[k]), np.asarray(off[k]), equal_nan=True), (case.id, k)
    assert on["iters_mean"] > 0.5


@pytest.mark.parametrize("case", REG, ids=_ids(REG))
def test_regulator_device_loop_equals_host_loop(case):
    """tmpc_reg_run (a solve launch and a reg_step_kernel launch per step) against per-step batch solves in numpy, on every
    regulator shape; some starts lie outside X and fail at step 0."""
    m, X, *_ = _solved(case)
    B, T = 128, 20
    x0 = X[np.random.default_rng(5).choice(len(X), B, replace=False)]
    w = np.random.default_rng(6).uniform(-0.05, 0.05, (B, T, 2))
    dev = m.run_closed_loop(x0, T, w=w, capture=0)
    host = rp.host_loop(m, x0, w, {"X": m._X, "U": m._U}, None)
    assert np.any(host["fail_step"] >= 0) and np.any(host["fail_step"] < 0)
    rp.compare_loops(dev, host)
