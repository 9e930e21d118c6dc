"""The masked factorisation and back substitution of csrc/tmpc_wave.hpp INSIDE the real kernels, at bit level: the product library against
lib/libtmpc_hip_select.so, the same source with -DTMPC_SELECT_FORMS in the wave kernel's translation units (csrc/Makefile) -- the
select forms that define the values, every other instruction as shipped.  The masked forms move no arithmetic, so every output of
every solve must be the same bits: the register allocation and the schedule around the inline assembly differ per instantiation,
and a DPP read of a stale register or a lane pattern off by one is an error of the size of an update, not of a rounding.

tests/select_free_end_to_end.py runs the cases -- four shapes, the fixture states with an infeasible and a zero-iteration row, a
warm-started closed loop that enters the refinement's working-set solves -- once per library, each in a process of its own (the
package binds its library at import), both at the same time.

The host execution model is not the reference here: its reciprocal (sim::rcp, a 14-bit seed) and v_rcp_f64 end within one ulp of 1 / x
after fast_rcp's Newton steps without being the same double, so a whole solve on the device is not bit-equal to the model's
(tests/test_wavesim.py holds the model to the oracle at 1e-8, tests/test_hip_parity.py the device)."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import common
import select_free_end_to_end as cases

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.fixture(scope="module")
def both(hip_lib, tmp_path_factory):
    select = os.path.join(common.PKG, "lib", "libtmpc_hip_select.so")
    if not os.path.exists(select):
        raise RuntimeError(f"{select} is missing: build it with `make -C {os.path.join(common.PKG, 'csrc')}`")
    d = str(tmp_path_factory.mktemp("select_free_e2e"))
    env = {k: v for k, v in os.environ.items() if k != "TMPC_LIB"}

    def run(side):
        path = os.path.join(d, side + ".npz")
        e = dict(env, TMPC_LIB=select) if side == "select" else env
        res = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "select_free_end_to_end.py"), path],
                             env=e, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, (side, res.stderr[-3000:])
        return dict(np.load(path))
    with ThreadPoolExecutor(2) as ex:
        product, sel = ex.map(run, ("product", "select"))
    return product, sel


@pytest.mark.parametrize("tag", list(cases.KERNELS))
def test_solves_are_bit_equal_to_the_select_forms(both, tag):
    product, sel = both
    assert str(product[tag + "/kernel"]) == cases.KERNELS[tag] == str(sel[tag + "/kernel"])
    st, it = product[tag + "/status"], product[tag + "/iters"]
    assert (st == 0).sum() >= 64                     # (solved instances, interior-point iterations and refinement taken)
    assert it[st == 0].max() >= 5
    if tag in ("cartpole-N10", "double_integrator-N5"):          # (the rows the parity tests know: infeasible, no iteration needed)
        assert (st == 2).any() and (it[st == 0] == 0).any()
    for k in cases.SOLVE_KEYS:
        a, b = product[f"{tag}/{k}"], sel[f"{tag}/{k}"]
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (tag, k, int((_bits(a) != _bits(b)).sum()))


@pytest.mark.parametrize("fused", ["on", "off"])
def test_warm_started_closed_loop_is_bit_equal_to_the_select_forms(both, fused):
    product, sel = both
    assert np.all(product[f"loop-{fused}/not_optimal"] == 0) and product[f"loop-{fused}/iters_sum"].sum() > 0
    for k in cases.LOOP_KEYS:
        a, b = product[f"loop-{fused}/{k}"], sel[f"loop-{fused}/{k}"]
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (fused, k, int((_bits(a) != _bits(b)).sum()))
