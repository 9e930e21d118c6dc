"""The naive reference of the closed loop's state machines (tests/glue_reference.py) where the truth is known, and the
batched numpy twins against it where it is not.  CPU only.

1. On the 36 trajectories recorded from the reference's own classes (nx = 4, nu = 1: glue_golden.npz, glue_smart_golden.npz)
   the naive reference reproduces the integers exactly and the floats to 1e-12 of the trajectory's scale.
2. BatchedEstimator / BatchedConsistentActuator (and the smart pair built from them as montecarlo.run_remote_tracking_mpc
   builds it) against the naive reference with several inputs and wide states: the shapes of glue_reference.SHAPES, loss
   rates 0, 0.3, 0.9, ancillary gain 0.8 K, dense non-symmetric A, B, K.  For nu > 1 the reference's own classes cannot be
   run past the end of a sequence, so this is the only judge of the twins there."""
import os

import numpy as np
import pytest

import common
import glue_reference as gr
from LinearMPCOverNetworks.Estimator import BatchedEstimator
from LinearMPCOverNetworks.SmartActuator import BatchedConsistentActuator

G = np.load(os.path.join(common.GOLDEN, "glue_golden.npz"))
GS = np.load(os.path.join(common.GOLDEN, "glue_smart_golden.npz"))
RECORDED = [("consistent" if str(c).startswith("e0") else "extended", str(c)) for c in G["cases"]] + [("smart", str(c)) for c in GS["cases"]]


def test_there_are_36_recordings():
    assert len(RECORDED) == 36 and len(set(RECORDED)) == 36


@pytest.mark.parametrize("kind,name", RECORDED, ids=[n for _, n in RECORDED])
def test_naive_reference_reproduces_the_reference_recordings(kind, name):
    Gz = GS if kind == "smart" else G
    g = lambda k: Gz[f"{name}/{k}"]                                       # noqa: E731
    out = gr.replay(kind, Gz["A"], Gz["B"], Gz["K"], None if kind == "smart" else Gz["Kp"], int(Gz["N"]),
                    g("U").transpose(0, 2, 1), g("theta"), g("gamma"), g("wv"), xn0=g("xn0") if kind == "extended" else None)
    want = dict(x=g("x"), x_hat=g("xhat"), x_nom=g("pkt_x") if kind == "smart" else g("xnom"), u=g("u"),
                s=g("s"), Theta=g("Theta"), q=g("q"))
    gr.compare({k: v[None] for k, v in out.items()}, {k: np.asarray(v)[None] for k, v in want.items()}, name)


def twin_replay(kind, model, case):
    """The batched twins driven as montecarlo.run_remote_tube_mpc / run_remote_tracking_mpc drive them, with given packets,
    every step recorded: the arrays of _native.mc_replay."""
    ext, smart = kind == "extended", kind == "smart"
    A, B, K, Kp, N = model["A"], model["B"], model["K"], model["K_anc"], model["N"]
    nb, T = case["theta"].shape
    x = case["x0"].copy()
    est = BatchedEstimator(A, B, K, x, N, K_plant=Kp if ext else None, robust=ext)
    act = BatchedConsistentActuator(A, B, K, np.zeros_like(K) if smart else Kp, x, is_extended_MPC_used=ext)
    out = {k: [] for k in ("x", "x_hat", "x_nom", "u", "s", "Theta", "q")}
    for t in range(T):
        q = est.get_qt()
        U_t = np.ascontiguousarray(case["U"][:, t].transpose(0, 2, 1))        # (B, nu, N+1)
        est.store(U_t)
        if ext:
            est.store_x_nom_0(case["xn0"][:, t])
        if smart:
            act.x_nom = x.copy()                                              # no nominal model: x_nom := x each step
        u, pk = act.process(U_t, q, x, case["theta"][:, t], case["xn0"][:, t] if ext else None)
        if smart:
            pk = {"x_t": x.copy(), "s_t": pk["s_t"]}
        out["x_nom"].append(np.array(pk["x_nom_t"] if ext else pk["x_t"]))
        x = x @ A.T + u @ B.T + case["w"][:, t]
        est.update(pk, case["gamma"][:, t])
        for k, v in (("x", x), ("x_hat", est.get_estimate()), ("u", u), ("s", act.s), ("Theta", act.Theta), ("q", q)):
            out[k].append(np.array(v))
    return {k: np.stack(v, axis=1) for k, v in out.items()}


# the table's horizons, and the ones the device handles are created with where they differ (glue_reference.horizon)
CASES = [(nx, nu, n, kind) for nx, nu, N in gr.SHAPES for kind in gr.KINDS for n in sorted({N, gr.horizon(nx, nu, N, kind)})]


@pytest.mark.parametrize("nx,nu,N,kind", CASES, ids=[f"nx{a}_nu{b}_N{c}_{k}" for a, b, c, k in CASES])
def test_batched_twins_equal_the_naive_reference(nx, nu, N, kind):
    model, case, want = gr.reference(nx, nu, N, kind)
    got = twin_replay(kind, model, case)
    gr.compare(got, want, f"twins nx={nx} nu={nu} N={model['N']} {kind}")
    gr.check_inputs(model, case, want)
