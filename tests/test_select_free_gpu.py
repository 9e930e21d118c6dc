"""The select-free factorisation and back substitution of csrc/tmpc_wave.hpp ON THE DEVICE -- the masked instructions themselves, through
lib/libtmpc_wavecheck.so (tests/wavecheck/wavecheck.hip: lanes_factor, lanes_backsub_lane, lanes_forward + lanes_backsub_lane with one
wave per problem) -- at N = 8, 11, 12, 16, every 16-lane row of the wave a matrix of its own, every output of all 64 lanes bit for bit:

* against the host execution model of the SELECT forms (tests/wavesim/selectfree_main.cpp, the `select` half of its output) on the same
  inputs.  The model's reciprocal is not the hardware's: sim::rcp is a 14-bit seed where v_rcp_f64 has a table of its own, and after
  fast_rcp's two Newton steps the two are each within one ulp of 1 / x (tests/test_wave_primitives_gpu.py::
  test_fast_rcp_is_within_one_ulp) without being the same double -- measured on random SPD matrices at N = 8: 5 of 64 values of 1 / d
  differ in the last place.  So the inputs are select_free_cases.dyadic_problems: matrices whose elimination is exact with power-of-two
  pivots, for which both reciprocals are exact, and arbitrary right-hand sides, so that every step of the substitutions still rounds.
  A wrong lane pattern or a stale DPP read is off by a whole entry on such inputs as on any other.
* against the SELECT forms on the device on random SPD matrices of condition 1 ... 1e8: lib/libtmpc_wavecheck_nofmac.so is the same
  source with -DTMPC_NO_DPP_FMAC, which compiles the select forms (and the compiler's two-instruction multiply-add: the same values).
* a pivot that is not positive at the first, a middle and the last step: flag, factor and 1 / d as the host model leaves them."""
import numpy as np
import pytest

import select_free_cases as sf
from test_wave_primitives_gpu import Harness

import hostsim  # noqa: E402  (tests/wavesim: test_wave_primitives_gpu puts it on sys.path)

pytestmark = pytest.mark.gpu

SIZES = [8, 11, 12, 16]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the plain host-model binary, built once"""
    return str(tmp_path_factory.mktemp("selectfree_gpu")), hostsim.build("selectfree", ["plain"])["selectfree"]


@pytest.fixture(scope="module")
def wc(hip_lib):
    h = Harness("libtmpc_wavecheck.so")
    assert h.lib.wavecheck_nofmac() == 0
    return h


@pytest.fixture(scope="module")
def wc_select(hip_lib):
    h = Harness("libtmpc_wavecheck_nofmac.so")
    assert h.lib.wavecheck_nofmac() == 1
    return h


def _same_in_every_row(got, want, keys, what):
    for key in keys:
        same = sf.bits(got[key]) == sf.bits(want[key])
        for r in range(4):          # every 16-lane row on its own, so that a failure names it
            assert np.all(same[:, 16 * r:16 * r + 16]), (what, key, "16-lane row", r, "differing values", int((~same[:, 16 * r:16 * r + 16]).sum()))


@pytest.mark.parametrize("n", SIZES)
def test_device_equals_the_host_model_of_the_select_forms(wc, host, n):
    d, exe = host
    rows, b1, b2 = sf.dyadic_problems(n)
    rc, err, forms = sf.run(exe, n, rows, b1, b2, d, f"dyadic_{n}")
    assert rc == 0, err[-2000:]
    dev = wc.lanes(n, rows, b1, b2)
    want = forms["select"]
    assert np.all(dev["ok"] == 1) and np.all(want["ok"] == 1.0)
    assert not np.array_equal(want["x"], np.round(want["x"] * 2.0 ** 20) / 2.0 ** 20)          # (the substitutions do round)
    _same_in_every_row(dev, want, ("dinv", "frows", "x", "x2"), n)


@pytest.mark.parametrize("n", SIZES)
def test_masked_forms_equal_the_select_forms_on_the_device(wc, wc_select, n):
    rows, b1, b2 = sf.random_problems(n, P=8)
    dev, sel = wc.lanes(n, rows, b1, b2), wc_select.lanes(n, rows, b1, b2)
    assert np.all(dev["ok"] == 1) and np.all(sel["ok"] == 1)
    _same_in_every_row(dev, sel, ("dinv", "frows", "x", "x2"), n)


@pytest.mark.parametrize("n", SIZES)
def test_device_reports_a_bad_pivot_like_the_host_model(wc, host, n):
    d, exe = host
    steps = [0, n // 2, n - 1]
    rows, b1, b2 = sf.dyadic_problems(n, P=3, seed=5, negative=steps)
    rc, err, forms = sf.run(exe, n, rows, b1, b2, d, f"pivot_{n}")
    assert rc == 0, err[-2000:]
    dev = wc.lanes(n, rows, b1, b2)
    assert np.all(dev["ok"] == 0) and np.all(forms["select"]["ok"] == 0.0), steps
    _same_in_every_row(dev, forms["select"], ("dinv", "frows", "x", "x2"), n)
