"""The case table of tests/test_shape_coverage.py (CPU) and tests/test_shape_parity.py (GPU): at least one problem for every
compiled instantiation of the wave-per-QP kernel (TMPC_SHAPES in csrc/tmpc_kernels.hip) and of the workgroup-per-QP kernel
(block tiles T = 1, 2, 4, 8), placed at the edges where padding and slot-boundary bugs live -- nv == NVP, the smallest nv that
selects a shape, single-row slots exactly full (rows == 64 DS), the first nv of a wider block tile.  NOT product code.

Each case names its builder (a tracking controller of common.make_mpc, or a double-integrator regulator with a k-gon X), the
kernel path it is solved on, the kernel instantiation and the condensed dimensions (nv, rows) expected for every variant, and a
state generator.  The dimensions are recorded, not derived: a change of the condensing or of pick_config that moves a case off
its edge fails tests/test_shape_coverage.py."""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

import common
from certificates import boundary_states
from LinearMPCOverNetworks.polytope_lite import Polytope
from LinearMPCOverNetworks.RegulatorMPC import RegulatorMPC

S = np.load(os.path.join(common.GOLDEN, "cartpole_N10_states.npy"))      # (x_k, ref) pairs of cart-pole closed loops

DI_A = np.array([[1.0, 1.0], [0.0, 1.0]])
DI_B = np.array([[0.0], [1.0]])
REG_SCALE = np.array([10.0, 2.0])


def facet_angles(k: int):
    """Normal directions of the k-gon, turned by a quarter step so that no facet is {x_1 <= c} (sin = 0): on x_1 such a row
    does not depend on u_0 and is checked once instead of kept, and the row count would not be (N - 1) k + ..."""
    return 2.0 * np.pi * (np.arange(k) + 0.25) / k


def polygon_X(k: int) -> Polytope:
    """k-gon circumscribed about the ellipse (x_1 / 10)^2 + (x_2 / 2)^2 = 1: facets a_i . (x_1 / 10, x_2 / 2) <= 1."""
    th = facet_angles(k)
    return Polytope(np.c_[np.cos(th) / REG_SCALE[0], np.sin(th) / REG_SCALE[1]], np.ones(k))


def input_box(rows: int) -> Polytope:
    """|u| <= 1 in `rows` rows: the two facets, then redundant copies at 1.5 (they keep their rows in the condensed QP, so the
    row count can be tuned to fill the single-row slots exactly)."""
    A = np.array([[1.0], [-1.0]] * ((rows + 1) // 2))[:rows]
    b = np.ones(rows)
    b[2:] = 1.5
    return Polytope(A, b)


def make_regulator(N: int, k: int, u_rows: int = 2, device: int = 0) -> RegulatorMPC:
    """Double-integrator RegulatorMPC (Q = I, R = 1) with X = polygon_X(k): (N - 1) k + N u_rows condensed rows."""
    m = RegulatorMPC(DI_A, DI_B, np.eye(2), np.eye(1), N)
    m.set_input_constraints(input_box(u_rows))
    m.set_state_constraints(polygon_X(k))
    m.set_device(device)
    m.generate_optimization_problem()
    return m


# ----------------------------------------------------------------------------------------------------------- state generators
def tracking_states(mpc, rng, n=256):
    """(X, R) for a tracking controller: interior / closed-loop states, states inside the region the terminal set reaches with
    one coordinate pushed to its edge, states on the edge of the tightened X itself, states outside it, and states at the
    steady state of their reference (the unconstrained minimiser is feasible: no iteration)."""
    nx = mpc._nx
    box = np.asarray(mpc._Xc.b[:nx], dtype=np.float64)
    cart = nx == 4
    n_in, n_bd, n_edge, n_out = 96, 64, 32, 32
    n_eq = n - n_in - n_bd - n_edge - n_out
    if cart:
        idx = rng.choice(len(S), n_in, replace=False)
        Xi, Ri = S[idx, :4], S[idx, 4:]
        reach = box * np.array([0.5, 0.4, 0.9, 0.5])
        r_amp = 2.0
    else:
        Xi = rng.uniform(-0.6, 0.6, (n_in, nx)) * box
        Ri = np.c_[rng.uniform(-0.8, 0.8, n_in) * box[0], np.zeros((n_in, nx - 1))]
        reach = box * np.array([1.0, 0.15])
        r_amp = 0.8 * box[0]
    Xb = np.r_[boundary_states(rng, reach, n_bd, 0.7), boundary_states(rng, box, n_edge, 0.97)]
    Xo = boundary_states(rng, box, n_out, 1.0)
    Xo[np.arange(n_out), rng.integers(0, nx, n_out)] *= rng.uniform(1.05, 1.5, n_out)
    r_eq = rng.uniform(-0.5, 0.5, n_eq) * box[0]
    Xe = np.c_[r_eq, np.zeros((n_eq, nx - 1))]
    X = np.r_[Xi, Xb, Xo, Xe]
    m = n_bd + n_edge + n_out
    R = np.r_[Ri, np.c_[rng.uniform(-r_amp, r_amp, m), np.zeros((m, nx - 1))], Xe]
    return X, R


def regulator_states(m, rng, n=256):
    """States of the polygon regulator: inside (on scaled ellipses), on the polygon's edges (many active rows; fast ones have
    no admissible input sequence), outside X, and at / near the origin (u = 0 or the unconstrained LQ inputs: no iteration)."""
    P = m._X
    k = P.A.shape[0]
    n_in, n_bd, n_out = 96, 96, 32
    n_eq = n - n_in - n_bd - n_out
    ph = rng.uniform(0, 2 * np.pi, n_in)
    Xi = rng.uniform(0.0, 0.9, n_in)[:, None] * np.c_[np.cos(ph), np.sin(ph)] * REG_SCALE
    # a point on facet i: the tangent point plus a step along the edge (|t| <= tan(pi / k) stays on the edge)
    th = facet_angles(k)[rng.integers(0, k, n_bd)]
    t = rng.uniform(-1, 1, n_bd) * np.tan(np.pi / k)
    Xb = np.c_[np.cos(th) - t * np.sin(th), np.sin(th) + t * np.cos(th)] * REG_SCALE * rng.uniform(0.995, 1.0, n_bd)[:, None]
    ph = rng.uniform(0, 2 * np.pi, n_out)
    Xo = rng.uniform(1.02, 1.5, n_out)[:, None] * np.c_[np.cos(ph), np.sin(ph)] * REG_SCALE
    Xe = rng.uniform(-1, 1, (n_eq, 2)) * np.array([0.05, 0.02]) * rng.choice([0.0, 1.0], n_eq)[:, None]
    return np.r_[Xi, Xb, Xo, Xe]


# ----------------------------------------------------------------------------------------------------------------- the table
@dataclass(frozen=True)
class Case:
    id: str
    kernels: tuple                 # expected kernel instantiation per variant, on `path`
    dims: tuple                    # expected (nv, condensed rows) per variant
    name: str = ""                 # tracking: workload of common.make_mpc
    N: int = 0
    fixed: bool = True
    extended: bool = False
    k: int = 0                     # regulator: facets of X
    u_rows: int = 2                # regulator: rows of U
    path: str = "auto"

    @property
    def regulator(self) -> bool:
        return self.k > 0

    @property
    def wave(self) -> bool:
        return all("::solve_kernel<" in n for n in self.kernels)

    def build(self, device: int = 0):
        """The controller, with its device problem (host-only for device = -1) and the kernel path set."""
        if self.regulator:
            m = make_regulator(self.N, self.k, self.u_rows, device)
        else:
            m, _ = common.make_mpc(self.name, self.N, self.fixed, extended=self.extended, create=True, device=device)
        if self.path != "auto":
            m.set_kernel_path(self.path)
        return m

    def states(self, m, n=256, seed=0):
        """(X, R, variant) -- R and variant None where the problem has none."""
        rng = np.random.default_rng(seed + 1000 * self.N + self.k)
        if self.regulator:
            return regulator_states(m, rng, n), None, None
        X, R = tracking_states(m, rng, n)
        if not self.extended:
            return X, R, None
        var = (rng.uniform(size=n) < 0.6).astype(np.uint8)
        # x_k of a gamma = 1 instance is the plant state: off the nominal state by an element of Z (-) W
        w = common.workload(self.name)["w_bound"]
        X = X + var[:, None] * rng.uniform(-1, 1, X.shape) * w * 3.0
        return X, R, var


def _w(nvp, dp, ds, kcp, cp, cs, wpb):
    return f"tmpc::solve_kernel<{nvp},{dp},{ds},{kcp},{cp},{cs},{wpb}>"


def _b(t):
    return f"tmpc::solve_block_kernel<{t}>"


def _di(N, kernel, nv, rows, fixed=False, path="auto", name="double_integrator"):
    return Case(f"{name}-{'fixed' if fixed else 'free'}-N{N}" + ("" if path == "auto" else f"-{path}"), (kernel,), ((nv, rows),),
                name=name, N=N, fixed=fixed, path=path)


def _cp(N, kernel, nv, rows, path="auto"):
    return Case(f"cartpole-N{N}" + ("" if path == "auto" else f"-{path}"), (kernel,), ((nv, rows),), name="cartpole", N=N, path=path)


def _ext(N, k0, d0, k1, d1):
    return Case(f"cartpole-ext-N{N}", (k0, k1), (d0, d1), name="cartpole", N=N, extended=True)


def _reg(N, k, kernel, rows, u_rows=2):
    return Case(f"regulator-N{N}-{k}gon" + ("" if u_rows == 2 else f"-u{u_rows}"), (kernel,), ((N, rows),), N=N, k=k, u_rows=u_rows)


CASES = [
    # all rows dense and single, nv <= 8 / 12 / 16: the double integrator (free x_0: Z rows; fixed x_0: none) and the regulator
    _di(3, _w(8, 0, 2, 0, 0, 0, 8), 6, 90),
    _di(5, _w(8, 0, 2, 0, 0, 0, 8), 8, 102),                                      # nv == NVP
    _reg(8, 16, _w(8, 0, 2, 0, 0, 0, 8), 128),                                   # single slots exactly full
    _reg(8, 17, _w(8, 0, 4, 0, 0, 0, 8), 135),                                   # first row count past two slots
    _reg(8, 34, _w(8, 0, 4, 0, 0, 0, 8), 254),
    _reg(8, 32, _w(8, 0, 4, 0, 0, 0, 8), 256, u_rows=4),                         # exactly full
    _di(9, _w(12, 0, 2, 0, 0, 0, 8), 10, 72, fixed=True),
    _di(9, _w(12, 0, 2, 0, 0, 0, 8), 12, 126),                                   # nv == NVP
    _reg(10, 12, _w(12, 0, 2, 0, 0, 0, 8), 128),                                 # exactly full
    _reg(12, 11, _w(12, 0, 4, 0, 0, 0, 4), 145),
    _reg(12, 21, _w(12, 0, 4, 0, 0, 0, 4), 255),
    _reg(12, 20, _w(12, 0, 4, 0, 0, 0, 4), 256, u_rows=3),                       # exactly full
    _di(13, _w(16, 0, 2, 0, 0, 0, 4), 14, 96, fixed=True),
    _di(15, _w(16, 0, 2, 0, 0, 0, 4), 16, 108, fixed=True),                      # nv == NVP
    _di(10, _w(16, 0, 2, 0, 0, 0, 4), 13, 126, name="double_integrator_darup"),
    _di(11, _w(16, 0, 4, 0, 0, 0, 4), 14, 138),
    _di(13, _w(16, 0, 4, 0, 0, 0, 4), 16, 150),                                  # nv == NVP
    # paired rows + factored block (the cart-pole)
    _cp(7, _w(11, 1, 0, 5, 4, 0, 8), 8, 474),                                     # smallest nv of the bench shape
    _cp(10, _w(11, 1, 0, 5, 4, 0, 8), 11, 504),                                   # nv == NVP
    _cp(11, _w(12, 1, 0, 5, 4, 0, 8), 12, 514),                                   # nv == NVP
    _cp(12, _w(22, 2, 0, 5, 4, 0, 4), 13, 524),
    _cp(21, _w(22, 2, 0, 5, 4, 0, 4), 22, 614),                                   # nv == NVP
    _cp(22, _w(24, 2, 0, 5, 4, 0, 4), 23, 624),
    _cp(23, _w(24, 2, 0, 5, 4, 0, 4), 24, 634),                                   # nv == NVP
    # the extended controller: both problems, the second one on the 4 x 7 factored block
    _ext(9, _w(11, 1, 0, 5, 4, 0, 8), (10, 494), _w(15, 1, 0, 4, 7, 0, 4), (14, 946)),
    _ext(10, _w(11, 1, 0, 5, 4, 0, 8), (11, 504), _w(15, 1, 0, 4, 7, 0, 4), (15, 956)),       # nv == NVP
    _ext(11, _w(12, 1, 0, 5, 4, 0, 8), (12, 514), _w(16, 1, 0, 4, 7, 0, 4), (16, 966)),       # nv == NVP, both
    _ext(12, _w(22, 2, 0, 5, 4, 0, 4), (13, 524), _w(26, 2, 0, 4, 7, 0, 4), (17, 976)),
    _ext(21, _w(22, 2, 0, 5, 4, 0, 4), (22, 614), _w(26, 2, 0, 4, 7, 0, 4), (26, 1066)),      # nv == NVP, both
    # workgroup-per-QP kernel: both ends of every tile (forced where the automatic choice is a wave shape)
    _cp(3, _b(1), 4, 434),
    _di(13, _b(1), 16, 150, path="block"),
    _di(14, _b(2), 17, 156),
    _di(29, _b(2), 32, 246),
    _cp(24, _b(2), 25, 644),
    _di(30, _b(4), 33, 252),
    _di(61, _b(4), 64, 438),
    _di(62, _b(8), 65, 444),
    _di(125, _b(8), 128, 822),
]
