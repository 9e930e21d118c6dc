"""The wave helpers of csrc/tmpc_wave.hpp AS SHIPPED, on the device: tests/wavecheck/wavecheck.hip wraps each of them in a kernel of one
64-lane wave per problem (lib/libtmpc_wavecheck.so, built by csrc/Makefile with the product's flags; lib/libtmpc_wavecheck_nofmac.so is
the same source with the compiler's two-instruction form of the DPP multiply-add).  tests/test_wave_swap_reduce.py and
tests/test_wavesim.py check the project's host model of these instructions; the whole-solve GPU tests run the helpers inside an
iteration that corrects itself.  Here every helper answers for itself:

  sums      swap_reduce_to_lds[_at], reduce_to_lds, wave_sum2, wave_reduce: within 64 * 2^-53 * sum|values| of math.fsum, every lane the
            same bits, and -- IEEE additions in an order the lane maps fix -- bit-equal to the host model (swapsum_main.cpp)
  fast_rcp  at most 1 ulp from the correctly rounded 1.0 / x, exact on powers of two
  vmax / vmin / vmax_abs  numpy.fmax / fmin on finite values, infinities, subnormals and quiet NaNs
  factor and solve  lanes_factor / lanes_forward / lanes_backsub_lane (N = 1 ... 16 in the DPP form, 17, 24, 28 with v_readlane) and
            rows32_factor_solve / rows32_resolve (N = 17, 22, 24, 26, 31, 32) against a long-double judge, with the same elimination in
            float64 numpy as the twin: e_dev <= 10 * max(e_twin, 1e-12 * max|x*|), the band of tests/test_sensitivity_gpu.py for "the
            same algorithm in another order and with fused multiply-adds".  Like there, the errors are maxima over the batch that
            shares a setting -- here the eight seeds of one (N, cond): the error of an ill-conditioned solve lies along one direction
            with a random coefficient, and the ratio of two single draws has no bound worth asserting.  A DPP read of a stale register
            is off by the size of an update, not by roundoff.

Surplus lanes: the kernels leave a COPY OF ROW 0 on the lanes >= N of a 16-lane row (tmpc_kernels.hip: `li = lane < NV ? lane : 0`),
with a zero right-hand side; the set-up here is that one.  Identity rows are what solve_working_set puts BELOW the rows of a working
set inside its MC x MC system (lanes < N): test_identity_rows_beyond_a_working_set.  block_chol and the LP kernel's own factor live in .hip files, not in the
header: they are not covered here."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import common
import sensitivity_reference as sr
import test_wave_swap_reduce as host_model

import hostsim  # noqa: E402  (tests/wavesim: test_wave_swap_reduce puts it on sys.path)

pytestmark = pytest.mark.gpu

LD = np.longdouble
L, MAXC = 64, 52
DPP_N = list(range(1, 17))
READLANE_N = [17, 24, 28]
ROWS32_N = [17, 22, 24, 26, 31, 32]
CONDS = [1.0, 1e4, 1e8, 1e11]
SEEDS = 8
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def _d(a):
    return a.ctypes.data_as(_dp)


class Harness:
    """ctypes binding of one harness library.  A missing library is an error, as for the product library."""

    def __init__(self, name):
        path = os.path.join(common.PKG, "lib", name)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with `make -C {os.path.join(common.PKG, 'csrc')}`")
        self.lib = C.CDLL(path)
        self.lib.wavecheck_sentinel.restype = C.c_double
        self.sentinel = self.lib.wavecheck_sentinel()

    def lanes(self, n, rows, b1, b2):
        """rows[P][64][n], b1 / b2[P][64]: what every lane holds"""
        P = rows.shape[0]
        assert rows.shape == (P, L, n) and b1.shape == (P, L) and b2.shape == (P, L)
        rows, b1, b2 = (np.ascontiguousarray(a, dtype=np.float64) for a in (rows, b1, b2))
        out = {"frows": np.empty((P, L, n)), "dinv": np.empty((P, L)), "x": np.empty((P, L)), "x2": np.empty((P, L)),
               "ok": np.empty((P, L), dtype=np.int32)}
        rc = self.lib.wavecheck_lanes(C.c_int(n), C.c_int(P), _d(rows), _d(b1), _d(b2), _d(out["frows"]), _d(out["dinv"]), _d(out["x"]),
                                      _d(out["x2"]), out["ok"].ctypes.data_as(_ip))
        assert rc == 0, ("wavecheck_lanes", n, rc)
        return out

    def rows32(self, n, M, b1, b2):
        P = M.shape[0]
        assert M.shape == (P, n, n) and b1.shape == (P, n) and b2.shape == (P, n)
        ldm = self.lib.wavecheck_rows32_ldm(C.c_int(n))
        assert ldm == ((n + 1) | 1)
        M, b1, b2 = (np.ascontiguousarray(a, dtype=np.float64) for a in (M, b1, b2))
        out = {"x": np.empty((P, n)), "fac": np.empty((P, n, ldm)), "x2": np.empty((P, n)), "ok": np.empty((P, L), dtype=np.int32)}
        rc = self.lib.wavecheck_rows32(C.c_int(n), C.c_int(P), _d(M), _d(b1), _d(b2), _d(out["x"]), _d(out["fac"]), _d(out["x2"]),
                                       out["ok"].ctypes.data_as(_ip))
        assert rc == 0, ("wavecheck_rows32", n, rc)
        return out

    def _sums(self, fn, args, data, cnt):
        data = np.ascontiguousarray(data, dtype=np.float64)
        assert data.shape[1:] == (MAXC, L)
        res = np.empty((data.shape[0], L, cnt))
        rc = fn(*args, _d(data), C.c_int(data.shape[0]), _d(res))
        assert rc == 0, (fn.__name__, args, rc)
        return res

    def swap_reduce(self, cnt, rr, data):
        return self._sums(self.lib.wavecheck_swap_reduce, (C.c_int(cnt), C.c_int(rr)), data, cnt)

    def swap_reduce_split(self, data):
        return self._sums(self.lib.wavecheck_swap_reduce_split, (), data, 42)

    def reduce(self, cnt, data):
        return self._sums(self.lib.wavecheck_reduce, (C.c_int(cnt),), data, cnt)

    def sum2(self, data):
        return self._sums(self.lib.wavecheck_sum2, (), data, 2)

    def wave_reduce(self, op, data):
        return self._sums(self.lib.wavecheck_wave_reduce, (C.c_int(op),), data, 1)[:, :, 0]

    def elementwise(self, op, a, b=None):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = a if b is None else np.ascontiguousarray(b, dtype=np.float64)
        assert a.shape == b.shape and a.ndim == 1
        r = np.empty_like(a)
        rc = self.lib.wavecheck_elementwise(C.c_int(op), _d(a), _d(b), C.c_int(a.size), _d(r))
        assert rc == 0, ("wavecheck_elementwise", op, rc)
        return r


@pytest.fixture(scope="module")
def wc(hip_lib):
    return Harness("libtmpc_wavecheck.so")


@pytest.fixture(scope="module")
def wc_nofmac(hip_lib):
    h = Harness("libtmpc_wavecheck_nofmac.so")
    assert h.lib.wavecheck_nofmac() == 1
    return h


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_sizes_that_are_not_compiled_are_refused(wc):
    z = np.zeros(MAXC * L)
    assert wc.lib.wavecheck_nofmac() == 0
    assert wc.lib.wavecheck_lanes(C.c_int(18), C.c_int(1), _d(z), _d(z), _d(z), _d(z), _d(z), _d(z), _d(z), None) == -2
    assert wc.lib.wavecheck_rows32(C.c_int(18), C.c_int(1), _d(z), _d(z), _d(z), _d(z), _d(z), _d(z), None) == -2
    assert wc.lib.wavecheck_swap_reduce(C.c_int(33), C.c_int(12), _d(z), C.c_int(1), _d(z)) == -2
    assert wc.lib.wavecheck_swap_reduce(C.c_int(44), C.c_int(16), _d(z), C.c_int(1), _d(z)) == -2
    assert wc.lib.wavecheck_reduce(C.c_int(2), _d(z), C.c_int(1), _d(z)) == -2
    assert wc.lib.wavecheck_wave_reduce(C.c_int(3), _d(z), C.c_int(1), _d(z)) == -2
    assert wc.lib.wavecheck_elementwise(C.c_int(4), _d(z), _d(z), C.c_int(1), _d(z)) == -2
    assert wc.lib.wavecheck_sum2(_d(z), C.c_int(0), _d(z)) == -3
    assert wc.lib.wavecheck_lanes(C.c_int(8), C.c_int(1 << 20), _d(z), _d(z), _d(z), _d(z), _d(z), _d(z), _d(z), None) == -3


# ---------------------------------------------------------------- sums

@pytest.fixture(scope="module")
def sums(tmp_path_factory):
    """the two data sets of tests/test_wave_swap_reduce.py and what the plain host-model binary of swapsum_main.cpp makes of them"""
    d = tmp_path_factory.mktemp("swapsum_gpu")
    sets = host_model._data_sets()
    inp = os.path.join(d, "in.bin")
    np.concatenate([s.ravel() for s in sets]).astype(np.float64).tofile(inp)
    # built on demand like there, plain (no sanitizer) and without optimisation: 3 s instead of 45, and the same bits -- the order of
    # the additions is in the lane maps (test_swap_reduce_is_deterministic_across_builds)
    exe = hostsim.build("swapsum", ["O0"])["swapsum_O0"]
    res = subprocess.run([exe, inp, os.path.join(d, "out.bin")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    model = host_model._split(np.fromfile(os.path.join(d, "out.bin"), dtype=np.float64), len(sets))
    return sets, np.stack(sets), model


def test_swap_reduce_totals_and_bits(wc, sums):
    sets, data, model = sums
    cases = [(rr, cnt) for rr in (12, 16) for cnt in range(1, 33)] + [(12, 44), (12, 52)]
    for rr, cnt in cases:
        got = wc.swap_reduce(cnt, rr, data)
        for s, vals in enumerate(sets):
            host_model._check(vals[:cnt], got[s])
            assert np.array_equal(_bits(got[s]), _bits(model[s][0][(rr, cnt)])), ("the host model gives other bits", rr, cnt, s)
    got = wc.sum2(data)
    for s, vals in enumerate(sets):
        host_model._check(vals[:2], got[s])
        assert np.array_equal(_bits(got[s]), _bits(model[s][1])), ("wave_sum2: the host model gives other bits", s)


def test_swap_reduce_with_a_split_output(wc, sums):
    """swap_reduce_to_lds_at as sweep B of the bench shape calls it: 34 totals, the first 22 to one LDS array and 12 to another"""
    sets, data, _ = sums
    got = wc.swap_reduce_split(data)
    for s, vals in enumerate(sets):
        assert np.all(got[s][:, 22:30] == wc.sentinel), "the gap between the two arrays was written"
        host_model._check(vals[:34], np.concatenate([got[s][:, :22], got[s][:, 30:]], axis=1))


def test_reduce_to_lds_totals(wc, sums):
    sets, data, _ = sums
    for cnt in (1, 15, 16, 17, 33):
        got = wc.reduce(cnt, data)
        for s, vals in enumerate(sets):
            host_model._check(vals[:cnt], got[s])


def test_wave_reduce_and_wave_sum2_over_many_vectors(wc, sums):
    """every one of the 2 x 52 value vectors as value 0 (and 1): OpSum within the fsum bound, OpMin / OpMax exact, all lanes agree"""
    sets, _, _ = sums
    rolled = np.stack([np.roll(vals, -c, axis=0) for vals in sets for c in range(MAXC)])
    vec = rolled[:, 0, :]
    got = wc.wave_reduce(0, rolled)
    for v, g in zip(vec, got):
        host_model._check(v[None], g[:, None])
    for op, ref in ((1, np.min), (2, np.max)):
        got = wc.wave_reduce(op, rolled)
        assert np.array_equal(_bits(got), _bits(np.repeat(ref(vec, axis=1)[:, None], L, axis=1))), op
    got = wc.sum2(rolled)
    for two, g in zip(rolled[:, :2, :], got):
        host_model._check(two, g)


# ---------------------------------------------------------------- fast_rcp, vmax, vmin, vmax_abs

def test_fast_rcp_is_within_one_ulp(wc):
    """Against 1.0 / x in float64 (correctly rounded).  Measured on an MI355X: see DESIGN.md."""
    rng = np.random.default_rng(5)
    pow2 = 2.0 ** np.arange(-1020, 1021).astype(np.float64)
    edge = np.array([1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52, 2.0 - 2.0 ** -52])
    rnd = (1.0 + rng.random(4096)) * 2.0 ** rng.integers(-1020, 1021, 4096).astype(np.float64)
    x = np.concatenate([pow2, -pow2, edge, -edge, rnd, -rnd])
    want = 1.0 / x
    assert np.all(np.isfinite(want)) and np.all(np.abs(want) >= 2.0 ** -1022)       # normal results throughout
    got = wc.elementwise(0, x)
    assert np.all(np.isfinite(got)) and np.array_equal(np.signbit(got), np.signbit(want))
    ulps = np.abs(_bits(got).astype(np.int64) - _bits(want).astype(np.int64))
    rest = ulps[2 * pow2.size:]
    print(f"fast_rcp: max {int(ulps.max())} ulp over {x.size} inputs; correctly rounded: {100.0 * np.mean(rest == 0):.2f} % of the "
          f"{rest.size} inputs that are no power of two, {100.0 * np.mean(ulps == 0):.2f} % of all")
    assert np.all(ulps[:2 * pow2.size] == 0), "a power of two is not exact"
    assert ulps.max() <= 1, (int(ulps.max()), x[np.argmax(ulps)])


def _same_up_to_zero_sign(got, want, a, b):
    """bit-equal, except NaN for NaN and, where a zero met the zero of the other sign, magnitudes only"""
    both_zero = (a == 0) & (b == 0) & (np.signbit(a) != np.signbit(b))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    plain = ~both_zero & ~nan
    assert np.array_equal(_bits(got[plain]), _bits(want[plain]))
    assert np.all(np.abs(got[both_zero]) == np.abs(want[both_zero]))


def test_vmax_vmin_vmax_abs(wc):
    rng = np.random.default_rng(6)
    sub = 5e-324
    special = np.array([0.0, -0.0, 1.0, -1.0, 2.5, -2.5, np.inf, -np.inf, sub, -sub, 1e-310, -1e-310, 2.0 ** -1022, 1.7e308, -1.7e308, np.nan])
    a = np.concatenate([np.repeat(special, special.size), rng.standard_normal(1000) * 10.0 ** rng.uniform(-300, 300, 1000)])
    b = np.concatenate([np.tile(special, special.size), rng.standard_normal(1000) * 10.0 ** rng.uniform(-300, 300, 1000)])
    with np.errstate(invalid="ignore"):
        _same_up_to_zero_sign(wc.elementwise(1, a, b), np.fmax(a, b), a, b)
        _same_up_to_zero_sign(wc.elementwise(2, a, b), np.fmin(a, b), a, b)
        _same_up_to_zero_sign(wc.elementwise(3, a, b), np.fmax(a, np.abs(b)), a, np.abs(b))
    # a quiet NaN in one operand: the other comes back; in both: NaN
    one = wc.elementwise(1, np.array([np.nan, 3.0, np.nan]), np.array([3.0, np.nan, np.nan]))
    assert one[0] == 3.0 and one[1] == 3.0 and np.isnan(one[2])
    one = wc.elementwise(3, np.array([np.nan, 3.0, np.nan]), np.array([-4.0, np.nan, np.nan]))
    assert one[0] == 4.0 and one[1] == 3.0 and np.isnan(one[2])


# ---------------------------------------------------------------- factor and solve

def _spd(n, cond, seed):
    rng = np.random.default_rng([n, int(round(math.log10(cond))), seed])
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(0.0, -math.log10(cond), n) if n > 1 else np.ones(1)
    a = (q * lam) @ q.T
    return 0.5 * (a + a.T), rng.standard_normal(n), rng.standard_normal(n)


def _ldl(A, b1, b2, dtype):
    """LDL' by Gaussian elimination without pivoting, the multipliers through the pivot's reciprocal, b1 carried along, b2 by forward
    substitution: the routines' algorithm in plain numpy (float64: the twin; longdouble: the judge of the factor)"""
    n = A.shape[0]
    M = np.array(A, dtype=dtype)
    y1, y2 = np.array(b1, dtype=dtype), np.array(b2, dtype=dtype)
    Lm = np.zeros((n, n), dtype=dtype)
    dinv = np.zeros(n, dtype=dtype)
    for k in range(n):
        dinv[k] = dtype(1) / M[k, k]
        f = M[k + 1:, k] * dinv[k]
        M[k + 1:, k + 1:] -= np.outer(f, M[k, k + 1:])
        y1[k + 1:] -= f * y1[k]
        Lm[k + 1:, k] = f
    for k in range(n - 1):
        y2[k + 1:] -= Lm[k + 1:, k] * y2[k]
    xs = []
    for y in (y1, y2):
        x = np.zeros(n, dtype=dtype)
        for i in range(n - 1, -1, -1):
            x[i] = y[i] * dinv[i]
            y[:i] -= M[:i, i] * x[i]
        xs.append(x)
    return Lm, dinv, xs[0], xs[1]


def _lay_lanes(n, mats, b):
    """mats[P][R][n][n], b[P][R][n] -> rows[P][64][n], rhs[P][64] as the kernels set the lanes up: row i of the matrix of a 16-lane
    row on its lane i (R = 4), or of the one matrix on lane i (R = 1); a copy of row 0 and a zero right-hand side on the other lanes"""
    P, R = mats.shape[:2]
    lane = np.arange(L)
    li = lane % 16 if R == 4 else lane
    r = lane // 16 if R == 4 else np.zeros(L, dtype=int)
    live = li < n
    src = np.where(live, li, 0)
    rows = mats[:, r, src, :]
    rhs = np.where(live[None, :], b[:, r, src], 0.0)
    return rows, rhs, r, li, live


def _lanes_run(h, n, mats, b1, b2):
    """the harness on a batch of matrices mats[m][n][n] (four to a wave in the DPP form); results per matrix"""
    R = 4 if n <= 16 else 1
    m = mats.shape[0]
    assert m % R == 0
    rows, r1, _, _, _ = _lay_lanes(n, mats.reshape(m // R, R, n, n), b1.reshape(m // R, R, n))
    _, r2, _, _, _ = _lay_lanes(n, mats.reshape(m // R, R, n, n), b2.reshape(m // R, R, n))
    out = h.lanes(n, rows, r1, r2)
    per = {}
    for key, v in out.items():
        v = v.reshape((m // R, R, L // R) + v.shape[2:])[:, :, :n]
        per[key] = v.reshape((m, n) + v.shape[3:])
    per["raw"] = out
    return per


@pytest.fixture(scope="module")
def problems():
    """per N: the matrices (cond fastest, then seed: a wave of the DPP form holds the four conditions of one seed), right-hand sides, the
    long-double judge and the float64 twin"""
    out = {}
    for n in sorted(set(DPP_N + READLANE_N + ROWS32_N)):
        A, b1, b2 = (np.array(v) for v in zip(*[_spd(n, c, s) for s in range(SEEDS) for c in CONDS]))
        judge = {"x": [], "x2": [], "mult": [], "dinv": []}
        twin = {"x": [], "x2": [], "mult": [], "dinv": []}
        for a, u, v in zip(A, b1, b2):
            xs = sr.ld_solve(a, np.stack([u, v], axis=1))
            Lj, dj, _, _ = _ldl(a, u, v, LD)
            judge["x"].append(xs[:, 0]); judge["x2"].append(xs[:, 1]); judge["mult"].append(Lj); judge["dinv"].append(dj)
            Lt, dt, xt, xt2 = _ldl(a, u, v, np.float64)
            twin["x"].append(xt); twin["x2"].append(xt2); twin["mult"].append(Lt); twin["dinv"].append(dt)
        out[n] = (A, b1, b2, {k: np.array(v) for k, v in judge.items()}, {k: np.array(v) for k, v in twin.items()})
    return out


def _rows32_run(h, n, A, b1, b2):
    o = h.rows32(n, A, b1, b2)
    tri = np.tril(np.ones((n, n), dtype=bool), -1)
    return {"x": o["x"], "x2": o["x2"], "mult": np.where(tri, o["fac"][:, :, :n], 0.0), "dinv": o["fac"][:, :, n], "ok": o["ok"], "raw": o}


def _lanes_outputs(h, n, A, b1, b2):
    o = _lanes_run(h, n, A, b1, b2)
    tri = np.tril(np.ones((n, n), dtype=bool), -1)
    return {"x": o["x"], "x2": o["x2"], "mult": np.where(tri, o["frows"], 0.0), "dinv": o["dinv"], "ok": o["raw"]["ok"], "raw": o["raw"]}


@pytest.fixture(scope="module")
def device_runs(wc, wc_nofmac, problems):
    """every factor / solve case through both libraries, once"""
    runs = {}
    for h, tag in ((wc, "dpp"), (wc_nofmac, "nofmac")):
        for n in DPP_N + READLANE_N:
            runs[("lanes", n, tag)] = _lanes_outputs(h, n, *problems[n][:3])
        for n in ROWS32_N:
            runs[("rows32", n, tag)] = _rows32_run(h, n, *problems[n][:3])
    return runs


def _band(routine, n, dev, judge, twin):
    """e_dev <= 10 * max(e_twin, 1e-12 * max|judge|) per output and condition number, the errors as maxima over the eight seeds"""
    worst = {}
    for key in ("x", "x2", "mult", "dinv"):
        for ci, cond in enumerate(CONDS):
            sel = np.arange(ci, len(judge[key]), len(CONDS))
            j = judge[key][sel]
            e_dev = float(np.max(np.abs(dev[key][sel].astype(LD) - j)))
            e_twin = float(np.max(np.abs(twin[key][sel].astype(LD) - j)))
            floor = 1e-12 * float(np.max(np.abs(j)))
            ratio = e_dev / max(e_twin, floor) if max(e_twin, floor) > 0 else (0.0 if e_dev == 0 else math.inf)
            worst[key] = max(worst.get(key, 0.0), ratio)
            assert np.all(np.isfinite(dev[key][sel])), (routine, n, key, cond)
            assert e_dev <= 10 * max(e_twin, floor), (routine, n, key, cond, e_dev, e_twin, floor)
    print(f"   {routine} N = {n}: worst e_dev / max(e_twin, floor): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    return worst


@pytest.mark.parametrize("form", ["dpp", "readlane"])
def test_lanes_factor_and_solves_against_the_judge(device_runs, problems, form):
    worst = {}
    for n in (DPP_N if form == "dpp" else READLANE_N):
        dev = device_runs[("lanes", n, "dpp")]
        assert np.all(dev["ok"] == 1), n
        for k, v in _band(f"lanes_* ({form})", n, dev, problems[n][3], problems[n][4]).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"lanes_factor / lanes_forward / lanes_backsub_lane, {form} form: worst ratios " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def test_rows32_factor_solve_and_resolve_against_the_judge(device_runs, problems):
    worst = {}
    for n in ROWS32_N:
        dev = device_runs[("rows32", n, "dpp")]
        assert np.all(dev["ok"] == 1), n
        for k, v in _band("rows32_*", n, dev, problems[n][3], problems[n][4]).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("rows32_factor_solve / rows32_resolve: worst ratios " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def test_dpp_form_and_compilers_form_give_the_same_bits(device_runs):
    """v_fmac_f64_dpp and fma(v_mov_b64_dpp(...)) round identically and `asm volatile` only fixes the order: every output of every
    case, on all 64 lanes, `ok` included"""
    for (routine, n, tag), run in device_runs.items():
        if tag != "dpp":
            continue
        other = device_runs[(routine, n, "nofmac")]["raw"]
        for key, v in run["raw"].items():
            if key == "ok":
                assert np.array_equal(v, other[key]), (routine, n, key)
            else:
                assert np.array_equal(_bits(v), _bits(other[key])), (routine, n, key)


def _same_bytes(a, b, what):
    for key in ("frows", "dinv", "x", "x2"):
        assert np.array_equal(_bits(a[key]), _bits(b[key])), (what, key)


@pytest.mark.parametrize("n", [1, 2, 5, 8, 11, 12, 15, 16])
def test_rows_of_the_wave_are_independent(wc, problems, n):
    """DPP forms: four different matrices on the four 16-lane rows (one seed's four condition numbers)"""
    A, b1, b2 = (v[:4] for v in problems[n][:3])
    mixed = _lanes_run(wc, n, A, b1, b2)
    assert np.all(mixed["raw"]["ok"] == 1)
    # each matrix alone: on all four rows of a wave of its own
    alone = _lanes_run(wc, n, np.repeat(A, 4, axis=0), np.repeat(b1, 4, axis=0), np.repeat(b2, 4, axis=0))
    for r in range(4):
        for copy in range(4):
            _same_bytes({k: mixed[k][r] for k in ("frows", "dinv", "x", "x2")},
                        {k: alone[k][4 * r + copy] for k in ("frows", "dinv", "x", "x2")}, (n, r, copy))
    # NaN and infinities on rows 1 - 3: row 0 keeps its bytes, and `ok` speaks for row 0 alone
    bad = A.copy()
    bad[1] = np.nan
    bad[2] = np.inf
    bad[3, 0, 0] = -np.inf
    bb1, bb2 = b1.copy(), b2.copy()
    bb1[1:] = [[np.nan], [np.inf], [-np.inf]]
    bb2[1:] = [[-np.inf], [np.nan], [np.inf]]
    hurt = _lanes_run(wc, n, bad, bb1, bb2)
    _same_bytes({k: mixed[k][0] for k in ("frows", "dinv", "x", "x2")}, {k: hurt[k][0] for k in ("frows", "dinv", "x", "x2")}, (n, "NaN"))
    assert np.all(hurt["raw"]["ok"] == 1)
    # the other way round: a matrix on row 0 that is not positive definite is what `ok` reports, whatever rows 1 - 3 hold
    worse = A.copy()
    worse[0] = -A[0]
    assert np.all(_lanes_run(wc, n, worse, b1, b2)["raw"]["ok"] == 0)


def _not_pd(n, k, pivot):
    """an integer matrix L D L' with unit lower triangular L (entries -1, 0, 1) and D of powers of two but D[k] = pivot: the elimination is
    exact, so pivot k IS `pivot` (0 or -1) on the device too"""
    rng = np.random.default_rng([n, k, int(pivot) + 7])
    Lm = np.tril(rng.integers(-1, 2, (n, n)).astype(np.float64), -1) + np.eye(n)
    d = 2.0 ** rng.integers(0, 3, n)
    d[k] = pivot
    return Lm @ np.diag(d) @ Lm.T


def _good(n):
    return np.eye(n) * 2.0


def test_lanes_factor_reports_a_pivot_that_is_not_positive(wc):
    for n in DPP_N + READLANE_N:
        R = 4 if n <= 16 else 1
        mats = []
        for k in sorted({0, n // 2, n - 1}):
            for pivot in (-1.0, 0.0):
                mats += [_not_pd(n, k, pivot)] + [_good(n)] * (R - 1)       # (the bad one on row 0, which is the row `ok` reports)
        mats = np.array(mats)
        b = np.ones(mats.shape[:2])
        ok = _lanes_run(wc, n, mats, b, b)["raw"]["ok"]
        assert np.all(ok == 0), (n, ok)


def test_rows32_factor_solve_leaves_everything_alone_on_a_bad_pivot(wc):
    for n in ROWS32_N:
        mats = np.array([_not_pd(n, k, pivot) for k in sorted({0, n // 2, n - 1}) for pivot in (-1.0, 0.0)] + [_good(n)])
        b = np.ones(mats.shape[:2])
        o = wc.rows32(n, mats, b, b)
        assert np.all(o["ok"][:-1] == 0) and np.all(o["ok"][-1] == 1), (n, o["ok"])
        assert np.all(o["x"][:-1] == wc.sentinel) and np.all(o["x2"][:-1] == wc.sentinel), n
        assert np.array_equal(_bits(o["fac"][:-1, :, :n]), _bits(mats[:-1])), (n, "the matrix in LDS was touched")
        assert np.all(o["fac"][:-1, :, n:] == wc.sentinel), n
        assert np.array_equal(o["x"][-1], np.full(n, 0.5)) and np.array_equal(o["x2"][-1], np.full(n, 0.5))
        assert np.array_equal(o["fac"][-1, :, n], np.full(n, 0.5))


@pytest.mark.parametrize("n,m", [(12, 1), (12, 5), (12, 11), (24, 13), (24, 22), (28, 7), (28, 26)])
def test_identity_rows_beyond_a_working_set(wc, problems, n, m):
    """solve_working_set's set-up (tmpc_kernels.hip: lanes_factor<MC> on a working set of m <= MC rows): S in the leading m x m block,
    identity rows beyond.  The leading block's solution is the m x m system's (judge: long double), the identity rows return their
    right-hand side, and what they hold as right-hand side (finite) does not reach the rows < m."""
    R = 4 if n <= 16 else 1
    pick = [4, 5, 6, 7] if R == 4 else [6]                  # (seed 1: its four condition numbers, or 1e8 alone)
    S, u, v = (a[pick] for a in problems[m][:3])
    A = np.tile(np.eye(n), (R, 1, 1))
    A[:, :m, :m] = S
    rng = np.random.default_rng([n, m])
    b1, b2 = rng.standard_normal((R, n)), rng.standard_normal((R, n))
    b1[:, :m], b2[:, :m] = u, v
    out = _lanes_run(wc, n, A, b1, b2)
    assert np.all(out["raw"]["ok"] == 1)
    assert np.array_equal(out["x"][:, m:], b1[:, m:]) and np.array_equal(out["x2"][:, m:], b2[:, m:])
    assert np.all(out["dinv"][:, m:] == 1.0) and np.all(out["frows"][:, m:, :m] == 0.0)
    for r in range(R):
        want = sr.ld_solve(S[r], np.stack([u[r], v[r]], axis=1))
        _, _, t1, t2 = _ldl(S[r], u[r], v[r], np.float64)
        for got, twin, w in ((out["x"][r, :m], t1, want[:, 0]), (out["x2"][r, :m], t2, want[:, 1])):
            e_dev, e_twin = float(np.max(np.abs(got.astype(LD) - w))), float(np.max(np.abs(twin.astype(LD) - w)))
            # One matrix, not a batch of eight: the twin's single draw is a fair yardstick only where the error is roundoff of the
            # data (cond <= 1e4); every case is held to the first-order bound of an LDL' solve, gamma_(3m+1) cond(S) with u = 2^-53
            # (Higham, Accuracy and Stability, Thm 10.4), sqrt(m) for the maximum norm.
            cond = CONDS[pick[r] % len(CONDS)]
            scale = float(np.max(np.abs(w)))
            if cond <= 1e4:
                assert e_dev <= 10 * max(e_twin, 1e-12 * scale), (n, m, r, e_dev, e_twin)
            assert e_dev <= 4 * m * math.sqrt(m) * cond * 2.0 ** -53 * scale, (n, m, r, e_dev, cond)
    other = _lanes_run(wc, n, A, np.concatenate([b1[:, :m], 1e3 * b2[:, m:]], axis=1), np.concatenate([b2[:, :m], -b1[:, m:]], axis=1))
    for key in ("frows", "dinv"):
        assert np.array_equal(_bits(out[key]), _bits(other[key])), (n, m, key)
    for key in ("x", "x2"):
        assert np.array_equal(_bits(out[key][:, :m]), _bits(other[key][:, :m])), (n, m, key)


@pytest.mark.parametrize("n", [1, 3, 8, 11, 12, 15, 17, 24, 28])
def test_surplus_lanes_do_not_reach_the_result(wc, problems, n):
    """what the lanes >= N hold as their right-hand side (finite) does not show on the lanes < N"""
    R = 4 if n <= 16 else 1
    A, b1, b2 = (v[:4] for v in problems[n][:3])
    mats = A.reshape(4 // R, R, n, n)
    rows, r1, _, li, live = _lay_lanes(n, mats, b1.reshape(4 // R, R, n))
    _, r2, _, _, _ = _lay_lanes(n, mats, b2.reshape(4 // R, R, n))
    assert not np.all(live)
    base = wc.lanes(n, rows, r1, r2)
    rng = np.random.default_rng(n)
    junk1 = np.where(live[None, :], r1, 1e6 * rng.standard_normal(r1.shape))
    junk2 = np.where(live[None, :], r2, 1e-6 * rng.standard_normal(r2.shape))
    other = wc.lanes(n, rows, junk1, junk2)
    for key in ("frows", "dinv", "x", "x2"):
        assert np.array_equal(_bits(base[key][:, live]), _bits(other[key][:, live])), (n, key)
    assert np.array_equal(base["ok"], other["ok"]) and np.all(base["ok"] == 1)
