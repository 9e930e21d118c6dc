"""Regulator MPC -- "from an initial condition bring the plant state to the origin" -- and parent of every MPC class of the package.

Drop-in for the reference module `LinearMPCOverNetworks.RegulatorMPC` (reference RegulatorMPC.py:11-94): constructor,
constraint setters, `generate_optimization_problem` / `solve_optimization_problem` and `set_solver`, the class the reference's
own modules import by this path (`TubeRegulatorMPC.py:12`, `TrackingMPC.py:16`).

What differs from the reference:

* `generate_optimization_problem` does not build a cvxpy problem (RegulatorMPC.py:45-76).  It hands the model, weights and
  the optional sets X and U to `tmpc_create_regulator` (include/tmpc.h), which condenses the QP once on the host
  (z = [u_0 .. u_{N-1}], x_0 = x_k) and keeps it resident in HBM.
* `solve_optimization_problem(x_init)` calls `tmpc_solve_batch` and returns `(x_mpc (nx, N+1), u_mpc (nu, N))`
  (RegulatorMPC.py:78-91), or `(None, None)` when the instance is infeasible (a state outside X).  Inputs may carry a
  leading batch axis, `(B, nx)`: the result is then `(x_mpc (B, N+1, nx), u_mpc (B, N, nu))` with NaN rows for the
  infeasible instances -- the batch layout of `TubeTrackingMPC`.
* `run_closed_loop` runs the loop of the reference's example script for a batch of trajectories on the device
  (`tmpc_reg_run`).

There is no CPU fall-back: without the HIP library `generate_optimization_problem` raises.
"""
from __future__ import annotations

import numpy as np

from .polytope_lite import as_polytope

STATUS_OPTIMAL = 0
STATUS_INFEASIBLE = 2
_STATUS_TEXT = {0: "optimal", 1: "optimal_inaccurate", 2: "infeasible", 3: "solver_error"}


class RegulatorMPC:
    """Reference RegulatorMPC.py:11-94."""

    _tube = False

    def __init__(self, A, B, Q, R, N: int) -> None:
        self._A = np.array(A, dtype=np.float64)
        self._B = np.array(B, dtype=np.float64)
        self._N = int(N)
        self._nx = self._A.shape[1]
        self._nu = self._B.shape[1]
        self._Q = np.array(Q, dtype=np.float64)
        self._R = np.atleast_2d(np.array(R, dtype=np.float64))
        self._X = None
        self._U = None
        # the reference stores cp.CLARABEL here (RegulatorMPC.py:31); this build has
        # exactly one back-end, the HIP library
        self._solver = "hip"
        self._handle = None
        self._device = 0
        self._tol = 1e-7
        self._max_iter = 60
        self.last_status = None
        self.last_iters = None

    def set_state_constraints(self, X) -> None:
        self._X = as_polytope(X)

    def set_input_constraints(self, U) -> None:
        self._U = as_polytope(U)

    def set_solver(self, solver) -> None:
        """Reference RegulatorMPC.py:93-94.  Only the HIP back-end exists here."""
        if str(solver).lower() not in ("hip", "clarabel"):
            raise ValueError("this build solves on the MI355X only (solver='hip')")
        self._solver = "hip"

    # ------------------------------------------------------------------ QP
    def _regulator_dict(self) -> dict:
        """Flat description handed across the C ABI (include/tmpc.h: tmpc_regulator_problem).  X / U = None: no rows."""
        d = dict(nx=self._nx, nu=self._nu, N=self._N, A=self._A, B=self._B, Q=self._Q, R=self._R, tube=0,
                 tol=self._tol, max_iter=self._max_iter)
        if self._X is not None:
            d["Hx"], d["hx"] = self._X.A, self._X.b
        if self._U is not None:
            d["Hu"], d["hu"] = self._U.A, self._U.b
        return d

    def generate_optimization_problem(self):
        """Build the device-resident QP (replaces RegulatorMPC.py:45-76)."""
        from . import _native
        self._close_regulator()
        self._handle = _native.create_regulator(self._regulator_dict(), self._device)

    def _is_batched(self, x) -> bool:
        """(nx,) and the reference's column vector (nx,1) are single instances; (B,nx) is a batch."""
        return np.ndim(x) == 2 and np.shape(x) != (self._nx, 1)

    def _solve_regulator(self, x_init) -> dict:
        from . import _native
        if self._handle is None:
            raise RuntimeError("generate_optimization_problem() has not been called")
        x = np.ascontiguousarray(np.asarray(x_init, dtype=np.float64).reshape(-1, self._nx))
        out = _native.solve_regulator_batch(self._handle, x)
        self.last_status, self.last_iters = out["status"], out["iters"]
        return out

    def solve_optimization_problem(self, x_init):
        """RegulatorMPC.py:78-91: (x_mpc (nx, N+1), u_mpc (nu, N)); batched over a leading axis when given one."""
        batched = self._is_batched(x_init)
        out = self._solve_regulator(x_init)
        if batched:
            return out["x_nom"], out["u_nom"]
        st = int(out["status"][0])
        if st != STATUS_OPTIMAL:
            print(f"Status of {'tube regulator' if self._tube else 'regulator'} MPC is: {_STATUS_TEXT.get(st, st)}")
        if st >= STATUS_INFEASIBLE:
            return None, None
        return out["x_nom"][0].T.copy(), out["u_nom"][0].T.copy()

    # ------------------------------------------------------------------ closed loop
    def _default_check_sets(self) -> dict:
        return {"X": self._X, "U": self._U}

    def _disturbance_bound(self):
        return None

    def run_closed_loop(self, x0, T: int, w=None, seed=None, first_trajectory: int = 0, w_bound=None, check_sets=None,
                        capture=None, plant=None) -> dict:
        """The loop of the reference's example scripts for a batch of trajectories, resident on the device
        (include/tmpc.h: tmpc_reg_run): per step one solve launch over all trajectories and one step-kernel launch that applies
        u_t = u_nom_0 - K (x_t - x_nom_0) (plain regulator: u_t = u_nom_0), updates x_{t+1} = A x_t + B u_t + w_t and sums the
        statistics.  x0 (B, nx) or (nx,).  w (B, T, nx) host disturbances; or, with `seed` given, w drawn on the device
        uniformly in the box of half-widths `w_bound` (default: the bounding box of the disturbance set W of the tube
        regulator) -- the stream of montecarlo.draw_realisations_philox(B, T, w_bound, seed, first_trajectory); neither: no
        disturbance.  check_sets: {"X": polytope, "U": ..., "Z": ...} (None entries: not checked; default: the
        un-tightened X and U, and Z for the tube regulator).  capture: index of one trajectory whose x_traj (T+1, nx),
        x_nom_traj (T, nx) and u_traj (T, nu) are returned.  plant: None, or a linear montecarlo.plant_family -- trajectory b then
        runs on x+ = A_b x + B_b u + w while the controller keeps its (A, B) (tmpc_mc_set_plant_models).
        Returns per trajectory cost (sum of x'Qx + u'Ru), x_viol, u_viol, tube_viol (steps outside the check sets),
        not_optimal, fail_step (first step with an infeasible solve, -1: none; the trajectory is frozen from there), x_final,
        iters_sum."""
        from . import _native
        if self._handle is None:
            raise RuntimeError("generate_optimization_problem() has not been called")
        x0 = np.asarray(x0, dtype=np.float64).reshape(-1, self._nx)
        sets = self._default_check_sets() if check_sets is None else dict(check_sets)
        device_rng = None
        if w is None and seed is not None:
            if w_bound is None:
                w_bound = self._disturbance_bound()
            if w_bound is None:
                raise ValueError("run_closed_loop: device-drawn disturbances need w_bound")
            device_rng = (int(seed), int(first_trajectory), np.asarray(w_bound, dtype=np.float64).reshape(self._nx))
        return _native.reg_run(self._handle, x0, T, w=w, device_rng=device_rng, X=sets.get("X"), U=sets.get("U"),
                               Z=sets.get("Z"), capture=capture, plant=plant)

    # ------------------------------------------------------------------ device and handle
    def set_device(self, device: int):
        self._device = int(device)

    def set_kernel_path(self, path: str):
        """'auto' (default) | 'wave' | 'block' -- include/tmpc.h: tmpc_set_kernel_path."""
        from . import _native
        _native.set_kernel_path(self._handle, path)

    def get_kernel_path(self, variant: int = 0) -> str:
        from . import _native
        return _native.get_kernel_path(self._handle, variant)

    def _close_regulator(self):
        if getattr(self, "_handle", None) is not None:
            from . import _native
            _native.destroy(self._handle)
            self._handle = None

    def _close(self):
        self._close_regulator()

    def __del__(self):
        try:
            self._close()
        except Exception:
            pass
