"""A naive, one-trajectory-at-a-time reference of the closed loop's state machines (NOT product code).

Written from the lines of the reference that include/tmpc.h and csrc/tmpc_mc_step.hpp cite -- SmartActuator.py:57-107 and
125-231, Estimator.py:43-161, the loop bodies results_linear_system.py:209-259, 262-287 and their counterpart in
results_linear_system_with_extendedMPC.py -- with plain Python loops over t and small numpy products on column vectors.
It imports nothing of the product's state machines (BatchedEstimator, BatchedConsistentActuator, montecarlo.run_remote_*):
it is the independent judge of the twins and of the device kernels.

Where the product keeps O(1) state per trajectory, this file keeps what the reference keeps: the whole list of arrival
flags (Theta_t is the product of the flags after q_t, SmartActuator.py:62-67) and every sequence ever sent (the estimator
looks up the one sent at s_t, Estimator.py:55).

Several inputs.  Past the end of a buffered sequence the reference's classes compute `u_sequ[:, -1] - K @ x` with a (nu,)
array against a (nu, 1) one, which broadcasts to (nu, nu) and fails at the following reshape for nu > 1: they cannot be run
there.  The intended law is the vector u_N - K x, which is what stands here (and for nu = 1 it is what the reference
computes: tests/test_glue_reference.py replays all 36 recorded reference trajectories).

`replay` takes what tmpc_mc_replay takes and returns what _native.mc_replay returns, for one trajectory.
`random_case` makes the inputs of the several-input tests (shape table SHAPES)."""
import numpy as np

KINDS = ("consistent", "extended", "smart")


def replay(kind, A, B, K, K_anc, N, U, theta, gamma, w, xn0=None, x0=None):
    """One trajectory.  kind: "consistent" (ConsistentActuator + Estimator), "extended" (ConsistentActuator in extended mode
    + RobustEstimator; needs xn0) or "smart" (plain SmartActuator + Estimator; K_anc is not used).
    U (T, N+1, nu): the controller's packets, terminal column last; theta, gamma (T,): arrival flags, both 1 at t = 0 (the
    first transmission always succeeds, results_linear_system.py:211-214); w (T, nx); xn0 (T, nx); x0 (nx,) or None (zero).
    Returns per step x (state after the step), x_hat (estimate after the step), x_nom (nominal state in the plant's
    packet; the measured state for the smart actuator), u (applied input), s, Theta, q (what the controller put into its
    packet)."""
    assert kind in KINDS
    A = np.asarray(A, dtype=np.float64)
    nx = A.shape[0]
    B = np.asarray(B, dtype=np.float64).reshape(nx, -1)
    nu = B.shape[1]
    K = np.asarray(K, dtype=np.float64).reshape(nu, nx)
    K_anc = None if kind == "smart" else np.asarray(K_anc, dtype=np.float64).reshape(nu, nx)
    U = np.asarray(U, dtype=np.float64)
    T = U.shape[0]
    assert U.shape == (T, N + 1, nu) and int(theta[0]) == 1 and int(gamma[0]) == 1
    col = lambda v, n: np.array(v, dtype=np.float64).reshape(n, 1)      # noqa: E731
    x = np.zeros((nx, 1)) if x0 is None else col(x0, nx)
    x_hat = x.copy()               # estimator
    x_nom = x.copy()               # nominal model on the plant side (not used by the smart actuator)
    q_est = 0                      # estimator: last step whose plant packet arrived
    sent = []                      # estimator: every sequence sent, (nu, N+1) each
    flags = []                     # actuator: every theta so far
    q_act, s, buffered = 0, 0, None
    out = dict(x=np.zeros((T, nx)), x_hat=np.zeros((T, nx)), x_nom=np.zeros((T, nx)), u=np.zeros((T, nu)),
               s=np.zeros(T, np.int64), Theta=np.zeros(T, np.int64), q=np.zeros(T, np.int64))
    for t in range(T):
        # ---- controller side: the packet {U_t, q_t [, x_nom_0]} is stored by the estimator whether it arrives or not
        q_sent = q_est
        U_t = U[t].T.copy()                                        # (nu, N+1)
        sent.append(U_t)
        xn0_t = col(xn0[t], nx) if kind == "extended" else None
        # ---- actuator: Theta_t, s_t, buffer
        th = int(theta[t])
        flags.append(th)
        if th == 1:
            q_act = q_sent
            Theta = 1
            for f in flags[q_act + 1:]:
                Theta *= f
        else:
            Theta = 0
        s = Theta * t + (1 - Theta) * s
        if Theta == 1:
            buffered = U_t
            if kind == "extended":
                x_nom = xn0_t.copy()
        # ---- input: inside the horizon the buffered column, past it the terminal law on the (nominal) state
        x_law = x if kind == "smart" else x_nom
        d = t - s
        if d < N:
            u_nom = buffered[:, d].reshape(nu, 1)
        else:
            u_nom = buffered[:, N].reshape(nu, 1) - K @ x_law
        if kind == "smart":
            u = u_nom
            pkt = {"x_t": x.copy(), "s_t": s}
        else:
            u = u_nom - K_anc @ (x - x_nom)
            if kind == "extended":
                pkt = {"x_t": x.copy(), "s_t": s, "x_nom_t": x_nom.copy()}
            else:
                pkt = {"x_t": x_nom.copy(), "s_t": s}
            x_nom = A @ x_nom + B @ u_nom
        out["x_nom"][t] = (pkt["x_nom_t"] if kind == "extended" else pkt["x_t"]).reshape(nx)
        # ---- plant
        x = A @ x + B @ u + col(w[t], nx)
        # ---- estimator
        if int(gamma[t]) == 1:
            seq = sent[pkt["s_t"]]
            x_ref = pkt["x_nom_t"] if kind == "extended" else pkt["x_t"]
            if t - pkt["s_t"] < N:
                u_hat = seq[:, t - pkt["s_t"]].reshape(nu, 1)
            else:
                u_hat = seq[:, N].reshape(nu, 1) - K @ x_ref
            if kind == "extended":
                u_hat = u_hat - K_anc @ (pkt["x_t"] - pkt["x_nom_t"])
            x_hat = A @ pkt["x_t"] + B @ u_hat
            q_est = t
        else:
            base = xn0_t if kind == "extended" else x_hat
            x_hat = A @ base + B @ sent[-1][:, 0].reshape(nu, 1)
        out["x"][t], out["x_hat"][t], out["u"][t] = x.reshape(nx), x_hat.reshape(nx), u.reshape(nu)
        out["s"][t], out["Theta"][t], out["q"][t] = s, Theta, q_sent
    return out


def replay_batch(kind, model, case):
    """`replay` over the trajectories of a batch (random_case): the arrays of _native.mc_replay, (B, T, ...)."""
    nb = case["U"].shape[0]
    runs = [replay(kind, model["A"], model["B"], model["K"], model["K_anc"], model["N"], case["U"][b], case["theta"][b],
                   case["gamma"][b], case["w"][b], xn0=case["xn0"][b], x0=case["x0"][b]) for b in range(nb)]
    return {k: np.stack([r[k] for r in runs], axis=0) for k in runs[0]}


# ---------------------------------------------------------------------------------------------------------- test inputs
# (nx, nu, N): what the shape is there for
SHAPES = [(3, 2, 4),       # smallest several-input case; B, K, K_anc dense and non-symmetric
          (2, 3, 5),       # nu > nx
          (7, 2, 6),       # nx past one Philox block boundary
          (12, 4, 30),     # BASELINE config 5: N nu = 120, second pass of the packet copy
          (16, 16, 5)]     # both limits, N nu = 80
P_LOSS = (0.0, 0.3, 0.9)
NB, T_STEPS = 12, 40


def horizon(nx, nu, N, kind):
    """The horizon a DEVICE handle of this shape and kind is created with, where tmpc_create refuses the table's own.
    (12, 4, 30) extended: the packet-received problem has a free initial state, nv = nx + (N + 1) nu = 136, and the compiled
    kernels end at nv = 128; N = 28 (nv = 128) keeps what the shape is there for, N nu = 112 > 64.
    (2, 3, 5): with nu > nx the matrix B has a null space, and along (u_k = u_bar = n, B n = 0) the tracking cost is constant:
    the condensed Hessian is singular in exact arithmetic, and whether its Cholesky factorisation in tmpc_create goes through
    is a matter of rounding.  With this model it does at N = 4 and does not at N = 5.  (No QP is solved with the handle.)"""
    if (nx, nu, N, kind) == (12, 4, 30, "extended"):
        return 28
    return 4 if (nx, nu, N) == (2, 3, 5) else N


def random_model(nx, nu, N, seed):
    """Dense A with spectral radius 0.9, dense B, K the LQR gain of (A, B, I, I) -- dense, non-symmetric, A - B K and
    A - 0.8 B K stable so that |x| stays small over the run -- and the ancillary gain 0.8 K."""
    from LinearMPCOverNetworks.control_lite import dlqr
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((nx, nx))
    A *= 0.9 / np.max(np.abs(np.linalg.eigvals(A)))
    B = rng.standard_normal((nx, nu))
    K, _, _ = dlqr(A, B, np.eye(nx), np.eye(nu))
    K = np.asarray(K, dtype=np.float64).reshape(nu, nx)
    for g in (K, 0.8 * K):
        assert np.max(np.abs(np.linalg.eigvals(A - B @ g))) < 0.98
    return dict(A=A, B=B, K=K, K_anc=0.8 * K, N=N, nx=nx, nu=nu)


def random_case(model, seed, nb=NB, T=T_STEPS):
    """Random packets and scripted losses for a batch: loss rates P_LOSS in turn, x0 non-zero.  The last trajectory (p = 0.9)
    loses every controller packet from t = 1 to t = N + 4 (where the run is long enough), so that its buffer is played
    past N whatever the draws; its plant packets arrive every other step there, so that the estimator's terminal law runs."""
    nx, nu, N = model["nx"], model["nu"], model["N"]
    rng = np.random.default_rng(seed)
    p = np.tile(P_LOSS, nb // len(P_LOSS))
    theta = (rng.uniform(size=(nb, T)) >= p[:, None]).astype(np.uint8)
    gamma = (rng.uniform(size=(nb, T)) >= p[:, None]).astype(np.uint8)
    hi = min(N + 5, T - 2)
    theta[-1, 1:hi] = 0
    gamma[-1, 1:hi] = np.arange(1, hi) % 2
    theta[:, 0] = gamma[:, 0] = 1
    return dict(p=p, theta=theta, gamma=gamma,
                U=0.3 * rng.standard_normal((nb, T, N + 1, nu)), xn0=0.5 * rng.standard_normal((nb, T, nx)),
                w=rng.uniform(-0.05, 0.05, (nb, T, nx)), x0=rng.standard_normal((nb, nx)))


def box_problem(model, extended):
    """The flat problem description (TubeTrackingMPC._problem_dict) of a model with plain box sets, for _native.create.  The
    replay solves nothing, so the sets need not be invariant."""
    nx, nu, N = model["nx"], model["nu"], model["N"]
    box = lambda n, r: (np.vstack([np.eye(n), -np.eye(n)]), np.full(2 * n, float(r)))      # noqa: E731
    Hx, hx = box(nx, 50.0)
    Hu, hu = box(nu, 20.0)
    HT, hT = box(2 * nx + nu, 40.0)
    d = dict(nx=nx, nu=nu, N=N, A=model["A"], B=model["B"], Q=np.eye(nx), R=np.eye(nu), P=2.0 * np.eye(nx), T=20.0 * np.eye(nx),
             K=model["K"], K_anc=model["K_anc"], Hx=Hx, hx=hx, Hu=Hu, hu=hu, HT=HT, hT=hT, fixed_x0=1, extended=0,
             tol=1e-7, max_iter=60)
    if extended:
        d["extended"] = 1
        d["HZW"], d["hZW"] = box(nx, 1.0)
        d["HTP"], d["hTP"] = box(nx + nu, 40.0)
    return d


FLOAT_TOL = 1e-12      # of the trajectory's scale: the same sums in another order (the band of tests/test_device_glue_replay.py)


def compare(got, want, label):
    """Integers exactly, floats to FLOAT_TOL of the trajectory's scale (max |x|, max |u| of the reference run, at least 1);
    arrays (B, T, ...).  Prints and returns the worst deviation."""
    for k in ("s", "Theta", "q"):
        assert np.array_equal(np.asarray(got[k], dtype=np.int64), np.asarray(want[k], dtype=np.int64)), (label, k)
    sx = np.maximum(np.abs(want["x"]).max(axis=(1, 2), keepdims=True), 1.0)
    su = np.maximum(np.abs(want["u"]).max(axis=(1, 2), keepdims=True), 1.0)
    err = {k: float(np.max(np.abs(got[k] - want[k]) / (su if k == "u" else sx))) for k in ("x", "x_hat", "x_nom", "u")}
    worst = max(err.values())
    print(f"   {label}: worst deviation / trajectory scale {worst:.2e} (" + ", ".join(f"{k} {v:.1e}" for k, v in err.items())
          + f"), max |x| {float(np.abs(want['x']).max()):.1f}")
    for k, v in err.items():
        assert v <= FLOAT_TOL, (label, k, v)
    return worst


_REFERENCE = {}


def reference(nx, nu, N, kind):
    """(model, inputs, the naive reference's trajectories) of one case, computed once and shared by the tests: read only."""
    key = (nx, nu, N, kind)
    if key not in _REFERENCE:
        model = random_model(nx, nu, N, seed=100 * nx + nu)
        case = random_case(model, seed=7 * nx + nu)
        _REFERENCE[key] = (model, case, replay_batch(kind, model, case))
    return _REFERENCE[key]


def check_inputs(model, case, want):
    """The inputs do what they are there for: all three loss rates, x0 non-zero, |x| moderate, consistent and inconsistent
    steps, and at p = 0.9 the buffer is played past its end."""
    assert set(case["p"]) == set(P_LOSS) and np.all(np.abs(case["x0"]).max(axis=1) > 0) and 1.0 < np.abs(want["x"]).max() < 1e3
    d = np.arange(want["s"].shape[1])[None, :] - want["s"]
    assert d[case["p"] == 0.9].max() >= model["N"] and d[case["p"] == 0.0].max() == 0
    assert (want["Theta"] == 0).any() and (want["Theta"] == 1).any()
