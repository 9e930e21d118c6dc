"""The register wave sums of csrc/tmpc_wave.hpp (wv::swap_reduce_to_lds: v_permlane32_swap / v_permlane16_swap halvings, then one
round of the transposition tile; wv::wave_sum2) on the host execution model of tests/wavesim/hip_sim.hpp.  CPU only.

What runs here is the project's MODEL of the instructions, not the instructions: in a host-model build wv::permlane_swap is an emulation
written from the manual and the DPP moves are hip_sim.hpp's.  This file checks the routine's lane maps and arithmetic on that model (and
its memory safety under the sanitizers); that the model and the hardware agree is tests/test_wave_primitives_gpu.py, which runs the same
cases on the device and compares the totals with this program's bit for bit.

For every count of values 1 ... 32 and both tile heights of the kernels (12 and 16 rows), and for the 44 and 52 values of sweep B at
N = 20 (12 rows; 52 values take two rounds of the tile), with random values and with values of
mixed signs and magnitudes (1e-12 ... 1e6): every total agrees with the float64 sum over the 64 lanes to within
64 * 2^-53 * sum |values| (only the order of the additions differs), and every lane reads the same totals.  The program is built
plain and, where the host toolchain has the runtimes, under ASan + UBSan and MSan (the tile and the outputs start out poisoned)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "wavesim"))
import hostsim  # noqa: E402

MAXC, L = 52, 64
KINDS = ("plain", "asan", "msan")


def _data_sets():
    rng = np.random.default_rng(11)
    plain = rng.standard_normal((MAXC, L))
    mixed = rng.choice([-1.0, 1.0], (MAXC, L)) * 10.0 ** rng.uniform(-12.0, 6.0, (MAXC, L))
    return [plain, mixed]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("swapsum")
    sets = _data_sets()
    inp = os.path.join(d, "in.bin")
    np.concatenate([s.ravel() for s in sets]).astype(np.float64).tofile(inp)
    exes = hostsim.binaries_or_skip(tmp_path_factory, "swapsum", KINDS, per_variant=True)
    out = {}
    for kind in KINDS:
        exe = exes.get(hostsim.names("swapsum", [kind])[0])
        if exe is None:          # the host toolchain lacks this sanitizer's runtime
            out[kind] = None
            continue
        res = subprocess.run([exe, inp, os.path.join(d, f"out_{kind}.bin")], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, **hostsim.SAN_ENV))
        assert res.returncode == 0, res.stderr[-4000:]
        hostsim.assert_clean(res.stderr)
        out[kind] = np.fromfile(os.path.join(d, f"out_{kind}.bin"), dtype=np.float64)
    return sets, out


def _split(raw, n_sets):
    """per data set: {(rr, cnt): [64][cnt]} and the [64][2] of wave_sum2"""
    parts, off = [], 0
    for _ in range(n_sets):
        red = {}
        for rr in (12, 16):
            for cnt in range(1, 33):
                red[(rr, cnt)] = raw[off:off + L * cnt].reshape(L, cnt)
                off += L * cnt
        for cnt in (44, 52):
            red[(12, cnt)] = raw[off:off + L * cnt].reshape(L, cnt)
            off += L * cnt
        s2 = raw[off:off + 2 * L].reshape(L, 2)
        off += 2 * L
        parts.append((red, s2))
    assert off == raw.size
    return parts


def _check(vals, got):
    """got[lane][c]: what each lane reads as the total of vals[c] over the lanes"""
    assert np.all(got == got[:1]), "the lanes read different totals"
    for c in range(got.shape[1]):
        exact = math.fsum(vals[c])
        bound = L * 2.0 ** -53 * float(np.sum(np.abs(vals[c])))
        assert abs(got[0, c] - exact) <= bound, (c, got[0, c], exact, bound)


@pytest.mark.parametrize("kind", list(KINDS))
def test_swap_reduce_totals_on_the_host_model(results, kind):
    sets, out = results
    if out[kind] is None:
        pytest.skip(f"the host toolchain has no {kind} runtime")
    for vals, (red, s2) in zip(sets, _split(out[kind], len(sets))):
        for (rr, cnt), got in red.items():
            _check(vals[:cnt], got)
        _check(vals[:2], s2)


def test_swap_reduce_is_deterministic_across_builds(results):
    """the order of the additions is fixed by the lane maps, not by the compiler: every build gives the same bits"""
    _, out = results
    built = [v for v in out.values() if v is not None]
    for v in built[1:]:
        assert np.array_equal(v, built[0])
