"""Tube regulator MPC of Mayne, Seron and Rakovic (2005), whose QP is solved on the MI355X; parent of the tube-tracking
controller.

Drop-in for the reference class `TubeRegulatorMPC` (TubeRegulatorMPC.py:14-163): the constructor
(:16-24: LQR gain `K`, terminal weight `P`, `Acl`), the mRPI driver with its s_max x10 retry (:26-78), `tighten_constraints`
(Uc = U (-) (-K)Z, Xc = X (-) Z, :80-89), `determine_Xf` (maximal output-admissible set of Acl on {Xc, -Kx in Uc}, :91-106),
`generate_optimization_problem` / `setup_optimization(W)` / `solve_optimization_problem(x_init)` (:108-160) and the
accessors `get_controller_gain` / `get_minimum_robust_positively_invariant_set`.

The QP (:109-143: z = (x_0, u), HZ (x_k - x_0) <= hZ, x_i in Xc, u_i in Uc, x_N in Xf, cost + x_N'P x_N) is condensed once by
`tmpc_create_regulator` (include/tmpc.h) and solved by the device kernels; `solve_optimization_problem` returns the reference's
`(x_mpc (nx, N+1), u_mpc (nu, N))` or `(None, None)`, batched as in `RegulatorMPC`.  `run_closed_loop` runs the loop of the
reference's example (u = u_nom_0 - K (x - x_nom_0), x+ = A x + B u + w) for a batch of trajectories on the device and counts
the steps that leave X, U and the tube x_nom_0 + Z.
"""
from __future__ import annotations

import numpy as np

from . import utils_polytope as up
from .RegulatorMPC import RegulatorMPC
from .control_lite import dlqr, dlyap
from .polytope_lite import Polytope, as_polytope, box_bounds, reduce


class TubeRegulatorMPC(RegulatorMPC):

    _tube = True

    def __init__(self, A, B, Q, R, N: int) -> None:
        super().__init__(A, B, Q, R, N)
        K, _, _ = dlqr(self._A, self._B, self._Q, self._R)      # TubeRegulatorMPC.py:19
        self._K = K
        Q_lyap = self._Q + K.T @ self._R @ K
        Q_lyap = (Q_lyap + Q_lyap.T) / 2
        self._Acl = self._A - self._B @ K
        # python-control convention  Acl P Acl^T - P + Q_lyap = 0  (TubeRegulatorMPC.py:23)
        self._P = dlyap(self._Acl, Q_lyap)
        self._Z = None
        self._W = None
        self._Xc = self._Uc = self._Xf = None

    def determine_mRPI(self, W, eps_var: float = 1.9e-5, Acl=None, rpi_method: int = 0, K=None):
        """Reference TubeRegulatorMPC.py:26-78."""
        if K is None:
            K = self._K
        if Acl is None:
            Acl = self._Acl
        if np.max(np.abs(np.linalg.eigvals(Acl))) >= 1:
            print("The matrix Acl is not stable, such that the algorithm will never converge. \n"
                  " Therefore, None is returned")
            return None
        s_max = 200
        while True:
            if rpi_method == 1:
                Fs_temp, status = up.calculate_RPI(Acl, W, self._X, self._U, K, eps_var=eps_var, s_max=s_max)
            else:
                if rpi_method != 0:
                    print("The method chosen to determine the RPI does not exists, so we use the default method 0")
                Fs_temp, status = up.calculate_minimal_robust_positively_invariant_set(
                    Acl, W=W, eps_var=eps_var, s_max=s_max)
            if status == 0:
                break
            if status == -2:
                raise ValueError("determine_mRPI: the disturbance set is too large for the state/input constraints "
                                 "(no RPI set fits inside them); the reference would retry with a larger s_max forever")
            if status == -3:
                raise ValueError("determine_mRPI: the container set of the Darup-Teichrib construction fails its contraction "
                                 "test for this model (independent of s_max); try rpi_method=0")
            print(f"RPI not determined in {s_max} steps. Increasing s_max to 10*s_max = {10 * s_max}")
            s_max *= 10
        self._Z = reduce(Fs_temp)
        return self._Z

    def tighten_constraints(self):
        """Uc = U (-) (-K) Z, Xc = X (-) Z  (TubeRegulatorMPC.py:80-89; equations (9), (10) of Mayne et al.)."""
        self._Uc = up.pont_diff(self._U, up.scale(self._Z, -self._K))
        self._Xc = up.pont_diff(self._X, self._Z)

    def determine_Xf(self, verbose: bool = True):
        """Maximal output-admissible set of x+ = Acl x on {x in Xc, -K x in Uc}  (TubeRegulatorMPC.py:91-106)."""
        Gxu = np.r_[self._Xc.A, -self._Uc.A @ self._K]
        fxu = np.r_[self._Xc.b, self._Uc.b]
        self._Xf = up.calculate_maximum_admissible_output_set(self._Acl, Polytope(Gxu, fxu), verbose=verbose)
        return self._Xf

    def _regulator_dict(self) -> dict:
        """include/tmpc.h: tmpc_regulator_problem with tube = 1 (TubeRegulatorMPC.py:109-143)."""
        d = dict(nx=self._nx, nu=self._nu, N=self._N, A=self._A, B=self._B, Q=self._Q, R=self._R, P=self._P, K=self._K, tube=1,
                 Hx=self._Xc.A, hx=self._Xc.b, Hu=self._Uc.A, hu=self._Uc.b, HZ=self._Z.A, hZ=self._Z.b,
                 tol=self._tol, max_iter=self._max_iter)
        if self._Xf is not None:
            d["Hf"], d["hf"] = self._Xf.A, self._Xf.b
        return d

    def generate_optimization_problem(self):
        """Build the device-resident QP (replaces TubeRegulatorMPC.py:108-143)."""
        if self._Z is None or self._Xc is None or self._Uc is None:
            raise RuntimeError("the tube regulator needs Z, Xc and Uc: call setup_optimization(W) (or determine_mRPI, "
                               "tighten_constraints, determine_Xf) first")
        super().generate_optimization_problem()

    def setup_optimization(self, W):
        """TubeRegulatorMPC.py:145-154: mRPI, tightened sets, terminal set, QP."""
        self._W = as_polytope(W)
        self.determine_mRPI(self._W)
        self.tighten_constraints()
        self.determine_Xf()
        self.generate_optimization_problem()

    def solve_optimization_problem(self, x_init):
        """TubeRegulatorMPC.py:156-160: (x_mpc (nx, N+1), u_mpc (nu, N)); x_mpc[:, 0] is the nominal state x_0."""
        return super().solve_optimization_problem(x_init)

    def get_controller_gain(self):
        """Gain of the ancillary controller u = u_nom - K (x - x_nom)  (TubeRegulatorMPC.py:162-164)."""
        return self._K

    def get_minimum_robust_positively_invariant_set(self):
        return self._Z

    def _default_check_sets(self) -> dict:
        return {"X": self._X, "U": self._U, "Z": self._Z}

    def _disturbance_bound(self):
        if self._W is None:
            return None
        bb = box_bounds(self._W)
        if bb is None:
            return None
        return np.maximum(np.abs(bb[0]), np.abs(bb[1]))
